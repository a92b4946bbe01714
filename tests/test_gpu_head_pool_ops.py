"""The classifier head, the loss and the pooling kernels one operator at a time, at the shapes where their tails are.

`linear_mfma_kernel`, `sgemm_mfma_strided_kernel`, `sgemm_strided_kernel`, `softmax_kernel`, the plain `ce_loss_kernel` (csrc/head.hip),
`maxpool_kernel` / `gavgpool_kernel` in bf16 and fp16 (csrc/pointwise.hip), `maxpool_idx_kernel`, `maxpool_bwd_kernel<3,2,1>`,
`maxpool_bwd_kernel<0,0,0>`, `maxpool3s2_bwd_pair_kernel`, `gavgpool_bwd_kernel` and `colsum_kernel`
(csrc/train_kernels.hip) run here through the single-operator hooks `spk_op_linear`, `spk_op_linear_backward`,
`spk_op_softmax`, `spk_op_cross_entropy`, `spk_op_maxpool`, `spk_op_maxpool_backward`, `spk_op_gavgpool` and
`spk_op_gavgpool_backward` (sykepic_hip/ops.py), which call the launchers the model executor and the training step call
(the Linear backward through `spk_linear_backward`, the one function both use).  Every reference is written out below in
int64 / float64 on the CPU; none calls the code under test.  No element of any output is left out of any check.

1. EXACT (`test_exact_*`): operands whose every partial sum is exactly representable, so the result must EQUAL the
   reference whatever the order of the sums.  Each test first asserts that on the reference: sum of |terms| < 2^24 for
   fp32 outputs, integers of at most 8 significant bits (|value| <= 256) for bf16 outputs.
   - Linear forward (x in [-3, 3], w in [-2, 2], b in [-4, 4], with and without bias): every `in` of LIN_IN_MFMA
     (`linear_mfma_kernel`: its float4 loop, the scalar K tail, waves without any K at in < 48) and of LIN_IN_GEMM (in % 4
     != 0: the strided GEMM) x every (n, out) of LIN_N_OUT (rows and columns clamped past the edge, one and several
     16 x 16 tiles).
   - Linear backward (gy, x in [-3, 3], w in [-2, 2]) in both forms (0: `sgemm_mfma_strided_kernel`, 1:
     `sgemm_strided_kernel`) and `colsum_kernel`: dw, db, dx against int64 matmuls for every n of LINB_N (K of the weight
     gradient: below / at / above 32, the zeroed tail) x every (out, in) of LINB_OUT_IN; then with each output null in
     turn.  The outputs live in one buffer filled with a sentinel, with guard bands between them: the outputs that were
     asked for equal the reference, every other float of the buffer (the skipped output, the guards) is untouched.
   - Max-pool forward, `maxpool_kernel` in bf16 and fp16 and `maxpool_idx_kernel`: values from multiples of 1/4 in
     [-3/4, 3/4] (three levels for the 1 x 2 and 2 x 2 images), and an all-negative tensor (a zero-initialised maximum
     fails it); at least 20 % of the windows of every case hold a tie (asserted).  Reference: pad with -inf, unfold the
     windows, the maximum, and for the saved tap THE SMALLEST tap number r * k + s among the taps equal to it.  k3 s2 p1 at
     POOL_HW x c 8 / 64 / 72 x n 1 / 3, and the four run-time forms of POOL_RT.
   - Max-pool backward (integer gy in [-8, 8]; at most 9 windows cover a pixel, |sum| <= 72): int64 scatter-add from the
     reference taps.  Even widths: form 0 (`maxpool_bwd_kernel<3,2,1>`), form 1 (`maxpool3s2_bwd_pair_kernel`) and form
     -1 each equal the reference; odd widths: form 0 / -1, form 1 is refused; POOL_RT: `maxpool_bwd_kernel<0,0,0>`.  Each
     with the taps the kernel saved and, separately, the reference's.
   - Global average pool (integers in [-3, 3]) for hw of GAP_HW x c of GAP_C x n 1 / 3, forward in bf16 and fp16 and
     backward: hw a power of two: equal; else forward |got - ref| <= 2^-23 |ref| (one rounding of 1 / hw, one of the
     product; the sum itself is exact), backward <= 2^-8 |ref| (those two, then one to bf16).
   - Softmax (base 1.3 and e) for c of SM_C x n 1 / 3 / 4 / 5: rows of equal logits give float32(1) * (float32(1) /
     float32(c)) exactly; a row with +1e4 at one index and -1e4 elsewhere gives exactly 1 there and 0 elsewhere.
   - Cross-entropy for c of SM_C x n of CE_N on integer logits: the count of correct rows is exact with ties planted
     between j and j + 1, j and j + 33 (different lanes) and j and j + 64 (the same lane), the label on the lower or the
     higher tied index; reference arg-max = the lowest index among the maxima.  Two calls on one `stats` add up (exactly
     twice); without dz the statistics are the same; c == 1: loss 0, dz 0.
2. BOUNDED (`test_random_*`): normal operands against float64 on the same fp32 / bf16 operands.  A = the float64 sum of
   the absolute values of the terms.  The bounds are derived from the kernels' arithmetic, none from what they give:
   - `linear_mfma_kernel`: (ceil(in / 4) + 4) 2^-24 A (four chains of in / 4 fused multiply-adds, a fixed tree);
   - the GEMM kernels: (K + 2) 2^-24 A;  `colsum_kernel`: (ceil(n / 8) + 4) 2^-24 A;
   - softmax: with e1 = 2 x 2^-24 max |z scale| + E the relative error of an exponential and t = (ceil(c / 64) + 7) 2^-24
     that of the sum and the reciprocal, |p - ref| <= (2 e1 + t) ref.  E = 3 ulp = 3 x 2^-23 is expf's own error: the
     OpenCL full-profile bound the ROCm device library is specified to meet (the ROCm installation ships no accuracy table
     of its own to cite).  scale = logf(base) from the C library, as the hook computes it;
   - cross-entropy, dz n: the same bound on p, plus 3 x 2^-24 |p - onehot| for the three roundings the softmax does not
     have (the subtraction, 1 / n, the product with it);
   - loss: per row e1 + t for log of the sum, plus 3 x 2^-23 |log s| for logf and 2^-24 (|lse| + |row loss|) for the two
     additions; then (n / 16 + 17) 2^-24 sum |row losses| for the two-level sum.
   Worst observed error / bound on an MI355X (printed by every bounded test): linear_mfma 0.08 (5 x 44 x 17), the GEMM as
   forward fallback 0.08, as dw / dx 0.12 in BOTH forms (the two kernels gave the same figures at every shape: each is a
   fused multiply-add chain in ascending k), colsum 0.03, softmax 0.16, dz n 0.46, loss 0.06.  None is above 1.

FOUND HERE: `softmax_kernel` wrote `expf(zr[j] * scale - mx)`, which the compiler contracts into one fma: the ROUNDED
maximum subtracted from the UNROUNDED product.  The maximum's own exponent was then a rounding residual instead of 0, so
its exponential was not 1, and a row of equal logits (z = 100 at base 1.3 and e, every c but 1 and 2) came out as
0.00099999981 instead of float32(1) / 1000.  The kernel's body is now compiled without contraction (one rounded product in
all three passes); the error was below the bound of the bounded test, so only `test_exact_softmax` saw it.  Its failing
shapes (n 4 and 5: the rows with z = 100 and z = -0.001) stay in the case list.  Every other kernel met every check at
the first run.

Not covered:
- Dropout (`test_head_dropout_trains` checks the mask statistics, the scale and the gradients);
- `predict_kernel` (covered against the golden) and the weight-pack kernels (an error there is gross);
- labels outside [0, c) and NaN propagation through max-pool;
- the grid-stride clamps (`grid_for`, 65535 blocks in y) need tensors of 10^8 elements and more.

Wall time of this file on an MI355X: 4.3 s for its 636 tests; the slowest is the first launch of the process (0.26 s),
every other test takes 0.02 s or less.
"""

import ctypes
import ctypes.util
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TWO24 = 2 ** 24
EPS = 2.0 ** -24
E_EXPF = 3 * 2.0 ** -23          # 3 ulp: the OpenCL full-profile bound for expf (and logf)
SENTINEL = -12345.0

# ---------------------------------------------------------------- cases
LIN_IN_MFMA = [4, 8, 44, 60, 64, 68, 100, 512, 516, 1280, 2560]
LIN_IN_GEMM = [1, 30, 49, 257]
# every n of {1, 5, 16, 17, 33} and every out of {1, 7, 16, 17, 49, 256}, a multiple of the tile only beside a ragged one
LIN_N_OUT = [(1, 7), (5, 1), (16, 17), (17, 16), (33, 49), (5, 256), (17, 49)]
LINB_N = [1, 3, 4, 5, 31, 32, 33, 64, 100]
LINB_OUT_IN = [(1, 30), (7, 4), (15, 33), (16, 31), (17, 32), (33, 100), (49, 512), (49, 31)]

POOL_HW = [(1, 2), (2, 2), (8, 8), (7, 8), (5, 6), (9, 7), (7, 7)]
POOL_S2 = [(n, h, w, c, 3, 2, 1) for (h, w) in POOL_HW for c in (8, 64, 72) for n in (1, 3)]
POOL_RT = [(n, h, w, c, k, s, p) for (k, s, p, h, w) in ((2, 2, 0, 6, 6), (3, 1, 1, 5, 7), (3, 2, 0, 7, 7), (5, 2, 2, 9, 8))
           for (n, c) in ((1, 8), (3, 72))]
POOL_CASES = POOL_S2 + POOL_RT

GAP_HW = [1, 2, 3, 4, 5, 49, 50, 196, 197]
GAP_C = [8, 64, 512, 520, 1280, 2048]
GAP_CASES = [(n, hw, c) for hw in GAP_HW for c in GAP_C for n in (1, 3)]

SM_C = [1, 2, 49, 63, 64, 65, 130, 1000]
SM_N = [1, 3, 4, 5]
CE_N = [1, 15, 16, 17, 33, 100]


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


# ---------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed), dtype=torch.int64)


def _normal(shape, seed, std=1.0):
    return (torch.randn(shape, generator=_gen(seed), dtype=torch.float32) * std).contiguous()


def _dev(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous()


def _assert_equal(got, exp, what):
    """got: device tensor; exp: CPU tensor of exactly representable values.  Equal as numbers (-0 == +0), NaN fails."""
    g = got.detach().cpu().double()
    e = exp.double().reshape(g.shape)
    bad = ~(g == e)
    nbad = int(bad.sum())
    if nbad:
        t = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements differ; first at {list(t)}: got {float(g[t])}, "
                             f"expected {float(e[t])}")


def _ratio(got, ref, bound, what):
    """Worst |got - ref| / bound over ALL elements (float64 on the CPU); printed, and asserted to be at most 1."""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (unwritten elements?)"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)    # (0 / 0: an exact element of bound 0)
    worst = float(ratio.max())
    i = int(ratio.argmax())
    print(f"[head_pool] {what}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (f"{what}: element {i} off by {float(err.flatten()[i]):.4e}, bound "
                          f"{float(bound.flatten()[i]):.4e} (ref {float(ref.flatten()[i]):.6e})")
    return worst


def _carve(shapes):
    """Float32 device buffer filled with SENTINEL holding one tensor per shape (None: a slot that stays unused), 64
    floats of guard band around each.  Returns (flat, views, mask of the floats that belong to no view)."""
    sizes = [0 if s is None else math.prod(s) for s in shapes]
    total = 64 + sum((sz + 63) // 64 * 64 + 64 for sz in sizes)
    flat = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    outside = torch.ones(total, dtype=torch.bool)
    views, off = [], 64
    for s, sz in zip(shapes, sizes):
        if s is None:
            views.append(None)
        else:
            views.append(flat[off:off + sz].view(*s))
            outside[off:off + sz] = False
        off += (sz + 63) // 64 * 64 + 64
    return flat, views, outside


def _assert_untouched(flat, outside, what):
    f = flat.cpu()
    assert bool((f[outside] == SENTINEL).all()), f"{what}: memory outside the requested outputs was written"


# ---------------------------------------------------------------- Linear forward
def _lin_ref(n, fin, fout, seed):
    x, w, b = _ints((n, fin), -3, 3, seed), _ints((fout, fin), -2, 2, seed + 1), _ints((fout,), -4, 4, seed + 2)
    y = x @ w.T
    assert int((x.abs() @ w.abs().T).max()) + 4 < TWO24
    return x, w, b, y


@pytest.mark.parametrize("n,fout", LIN_N_OUT, ids=_ids(LIN_N_OUT))
@pytest.mark.parametrize("fin", LIN_IN_MFMA + LIN_IN_GEMM)
def test_exact_linear_forward(fin, n, fout):
    from sykepic_hip import ops
    x, w, b, y = _lin_ref(n, fin, fout, 1000 * fin + 10 * n + fout)
    xd, wd = _dev(x), _dev(w)
    _assert_equal(ops.linear(xd, wd, None), y, "y without bias")
    _assert_equal(ops.linear(xd, wd, _dev(b)), y + b, "y with bias")


@pytest.mark.parametrize("n,fin,fout", [(33, 516, 49), (17, 2560, 7), (5, 44, 17), (17, 257, 49), (33, 30, 17)],
                         ids=lambda v: str(v))
def test_random_linear_forward(n, fin, fout):
    from sykepic_hip import ops
    x, w, b = _normal((n, fin), 1), _normal((fout, fin), 2, 0.5), _normal((fout,), 3)
    ref = x.double() @ w.double().T + b.double()
    A = x.double().abs() @ w.double().abs().T + b.double().abs()
    steps = (fin + 3) // 4 + 4 if fin % 4 == 0 else fin + 2          # linear_mfma_kernel / the GEMM (K = in)
    kernel = "linear_mfma" if fin % 4 == 0 else "sgemm (forward fallback)"
    _ratio(ops.linear(_dev(x), _dev(w), _dev(b)), ref, steps * EPS * A, f"{kernel} {n}x{fin}x{fout}")


# ---------------------------------------------------------------- Linear backward
LINB_CASES = [(n, fout, fin) for n in LINB_N for (fout, fin) in LINB_OUT_IN]


def _linb_run(ops, gy, x, w, want, form):
    """want: which of (dw, db, dx) are asked for.  Returns the views (None where skipped) after checking the guards."""
    n, fout = gy.shape
    fin = x.shape[1]
    shapes = [(fout, fin), (fout,), (n, fin)]
    flat, views, outside = _carve(shapes)
    passed = [v if k else None for v, k in zip(views, want)]
    for v, k in zip(views, want):          # a skipped output's slot counts as outside
        if not k:
            off = v.data_ptr() - flat.data_ptr()
            outside[off // 4: off // 4 + v.numel()] = True
    ops.linear_backward(gy, x, w, dw=passed[0], db=passed[1], dx=passed[2], form=form)
    _assert_untouched(flat, outside, f"form {form} want {want}")
    return passed


@pytest.mark.parametrize("form", [0, 1], ids=["mfma", "fma"])
@pytest.mark.parametrize("n,fout,fin", LINB_CASES, ids=_ids(LINB_CASES))
def test_exact_linear_backward(n, fout, fin, form):
    from sykepic_hip import ops
    seed = 100000 * n + 100 * fin + fout
    gy, x, w = _ints((n, fout), -3, 3, seed), _ints((n, fin), -3, 3, seed + 1), _ints((fout, fin), -2, 2, seed + 2)
    dw, db, dx = gy.T @ x, gy.sum(0), gy @ w
    assert int((gy.abs().T @ x.abs()).max()) < TWO24 and int(gy.abs().sum(0).max()) < TWO24
    assert int((gy.abs() @ w.abs()).max()) < TWO24
    gyd, xd, wd = _dev(gy), _dev(x), _dev(w)
    refs = (dw, db, dx)
    for want in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        got = _linb_run(ops, gyd, xd, wd, want, form)
        for g, r, name in zip(got, refs, ("dw", "db", "dx")):
            if g is not None:
                _assert_equal(g, r, f"{name} (form {form}, outputs {want})")


@pytest.mark.parametrize("form", [-1, 0, 1], ids=["production", "mfma", "fma"])
@pytest.mark.parametrize("n,fout,fin", [(100, 49, 100), (33, 17, 31)], ids=lambda v: str(v))
def test_random_linear_backward(n, fout, fin, form):
    from sykepic_hip import ops
    gy, x, w = _normal((n, fout), 4), _normal((n, fin), 5), _normal((fout, fin), 6, 0.5)
    g64, x64, w64 = gy.double(), x.double(), w.double()
    dw, db, dx = _linb_run(ops, _dev(gy), _dev(x), _dev(w), (1, 1, 1), form)
    name = {-1: "sgemm production", 0: "sgemm_mfma_strided", 1: "sgemm_strided (FMA)"}[form]
    _ratio(dw, g64.T @ x64, (n + 2) * EPS * (g64.abs().T @ x64.abs()), f"{name} dw K={n}")
    _ratio(dx, g64 @ w64, (fout + 2) * EPS * (g64.abs() @ w64.abs()), f"{name} dx K={fout}")
    _ratio(db, g64.sum(0), ((n + 7) // 8 + 4) * EPS * g64.abs().sum(0), f"colsum n={n}")


# ---------------------------------------------------------------- max-pool
@functools.lru_cache(maxsize=None)
def _pool_ref(case, negative):
    """Quarter-valued x [n,h,w,c] (float32 values exact in bf16 and fp16), and the reference written out: windows over the
    -inf padded image; y = their maximum; idx = the smallest tap number r * k + s among the taps equal to the maximum;
    gy integer in [-8, 8] and gx = the int64 scatter-add of gy at the pixel each saved tap points at."""
    n, h, w, c, k, stride, pad = case
    levels = 3 if h * w <= 4 else 7
    seed = sum(v * m for v, m in zip(case, (1, 10, 100, 1000, 7919, 104729, 1299709))) + (7 if negative else 0)
    q = _ints((n, h, w, c), 0, levels - 1, seed)
    x = (-(q + 1) if negative else q - levels // 2).double() / 4
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = F.pad(x.permute(0, 3, 1, 2), (pad, pad, pad, pad), value=float("-inf"))
    win = F.unfold(xp, k, stride=stride).reshape(n, c, k * k, ho, wo)        # tap index r * k + s, row-major
    y = win.max(dim=2).values
    ismax = win == y.unsqueeze(2)
    taps = torch.arange(k * k).reshape(1, 1, k * k, 1, 1)
    idx = torch.where(ismax, taps, torch.full_like(taps, k * k)).min(dim=2).values
    assert int(idx.max()) < k * k and bool(torch.isfinite(y).all())
    tie_fraction = float((ismax.sum(2) >= 2).double().mean())
    y, idx = y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous()      # NHWC
    gy = _ints((n, ho, wo, c), -8, 8, seed + 1)
    gx = _pool_scatter(gy, idx, (n, h, w, c), k, stride, pad)
    gxa = _pool_scatter(gy.abs(), idx, (n, h, w, c), k, stride, pad)
    assert int(gxa.max()) <= 256
    return x.float(), y, idx, tie_fraction, gy, gx


def _pool_scatter(gy, idx, in_shape, k, stride, pad):
    n, h, w, c = in_shape
    _, ho, wo, _ = gy.shape
    img = torch.arange(n).reshape(n, 1, 1, 1).expand_as(gy)
    iy = torch.arange(ho).reshape(1, ho, 1, 1) * stride - pad + idx // k
    ix = torch.arange(wo).reshape(1, 1, wo, 1) * stride - pad + idx % k
    ch = torch.arange(c).reshape(1, 1, 1, c).expand_as(gy)
    assert int(iy.min()) >= 0 and int(iy.max()) < h and int(ix.min()) >= 0 and int(ix.max()) < w
    gx = torch.zeros(in_shape, dtype=torch.int64)
    gx.index_put_((img, iy.expand_as(gy), ix.expand_as(gy), ch), gy, accumulate=True)
    return gx


@pytest.mark.parametrize("negative", [False, True], ids=["mixed", "negative"])
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_exact_maxpool_forward(case, negative):
    from sykepic_hip import ops
    n, h, w, c, k, stride, pad = case
    x, y, idx, ties, _, _ = _pool_ref(case, negative)
    assert ties >= 0.2, f"only {ties:.0%} of the windows hold a tie: the case does not test the tie rule"
    if negative:
        assert float(x.max()) < 0
    for dt in (torch.bfloat16, torch.float16):
        got, _ = ops.maxpool(_dev(x, dt), k, stride, pad)
        _assert_equal(got, y, f"maxpool_kernel {dt}")
    got, gidx = ops.maxpool(_dev(x, torch.bfloat16), k, stride, pad, want_idx=True)
    _assert_equal(got, y, "maxpool_idx_kernel y")
    _assert_equal(gidx, idx, "maxpool_idx_kernel saved tap")


@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_exact_maxpool_backward(case):
    from sykepic_hip import ops
    n, h, w, c, k, stride, pad = case
    x, _, idx, _, gy, gx = _pool_ref(case, False)
    _, own = ops.maxpool(_dev(x, torch.bfloat16), k, stride, pad, want_idx=True)
    gyd = _dev(gy, torch.bfloat16)
    pair = (k, stride, pad) == (3, 2, 1) and w % 2 == 0
    for name, taps in (("the kernel's taps", own), ("the reference taps", _dev(idx, torch.uint8))):
        for form in (-1, 0, 1):
            if form == 1 and not pair:
                with pytest.raises(RuntimeError, match="pixel-pair"):
                    ops.maxpool_backward(gyd, taps, (h, w), k, stride, pad, form=1)
                continue
            _assert_equal(ops.maxpool_backward(gyd, taps, (h, w), k, stride, pad, form=form), gx,
                          f"gx, form {form}, {name}")


# ---------------------------------------------------------------- global average pool
def _is_pow2(v):
    return v & (v - 1) == 0


@pytest.mark.parametrize("n,hw,c", GAP_CASES, ids=_ids(GAP_CASES))
def test_exact_gavgpool(n, hw, c):
    from sykepic_hip import ops
    x = _ints((n, hw, c), -3, 3, 1000 * hw + c + n)
    assert int(x.abs().sum(1).max()) < TWO24
    ref = x.sum(1).double() / hw
    for dt in (torch.bfloat16, torch.float16):
        got = ops.gavgpool(_dev(x, dt))
        if _is_pow2(hw):
            _assert_equal(got, ref, f"gavgpool_kernel {dt}")
        else:
            err = (got.cpu().double() - ref).abs()
            assert bool((err <= 2.0 ** -23 * ref.abs()).all()), f"gavgpool_kernel {dt}: worst {float(err.max()):.3e}"
    gy = _ints((n, c), -3, 3, 1000 * hw + c + n + 1)
    refb = (gy.double() / hw).unsqueeze(1).expand(n, hw, c)
    got = ops.gavgpool_backward(_dev(gy), hw)
    if _is_pow2(hw):
        _assert_equal(got, refb, "gavgpool_bwd_kernel")
    else:
        err = (got.cpu().double() - refb).abs()
        assert bool((err <= 2.0 ** -8 * refb.abs()).all()), f"gavgpool_bwd_kernel: worst {float(err.max()):.3e}"


# ---------------------------------------------------------------- softmax
def _logf(v):
    """logf of the C library: the scale the hook (and the model executor) hands the kernel for a base."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    return float(libm.logf(v))


SM_CASES = [(n, c) for c in SM_C for n in SM_N]


@pytest.mark.parametrize("base", [1.3, math.e], ids=["base1.3", "base_e"])
@pytest.mark.parametrize("n,c", SM_CASES, ids=_ids(SM_CASES))
def test_exact_softmax(n, c, base):
    from sykepic_hip import ops
    # rows of equal logits (a different constant per row)
    z = torch.tensor([-7.5, 0.0, 3.25, 100.0, -0.001])[:n].reshape(n, 1).expand(n, c).contiguous()
    one = torch.tensor(1.0, dtype=torch.float32)
    expect = (one * (one / torch.tensor(float(c), dtype=torch.float32))).expand(n, c)
    _assert_equal(ops.softmax(_dev(z), base), expect, "softmax of equal logits")
    # one logit 2e4 above the others: exp underflows to an exact 0 for them
    z = torch.full((n, c), -1e4)
    hot = torch.tensor([(37 * r + c // 2) % c for r in range(n)])
    z[torch.arange(n), hot] = 1e4
    expect = torch.zeros((n, c))
    expect[torch.arange(n), hot] = 1.0
    _assert_equal(ops.softmax(_dev(z), base), expect, "softmax of a +-1e4 row")       # (NaN / inf fail the equality)


def _softmax_ref(z, scale):
    """float64 softmax of z * scale and the bound of the module docstring, per element."""
    zs = z.double() * scale
    c = z.shape[1]
    e = torch.exp(zs - zs.max(1, keepdim=True).values)
    s = e.sum(1, keepdim=True)
    e1 = 2 * EPS * zs.abs().max(1, keepdim=True).values + E_EXPF
    t = ((c + 63) // 64 + 7) * EPS
    return e / s, e1, t, zs, s


@pytest.mark.parametrize("n,c", [(5, 1000), (3, 49), (4, 130)], ids=lambda v: str(v))
def test_random_softmax(n, c):
    from sykepic_hip import ops
    z = _normal((n, c), 7, 4.0)
    p, e1, t, _, _ = _softmax_ref(z, _logf(1.3))
    _ratio(ops.softmax(_dev(z), 1.3), p, (2 * e1 + t) * p, f"softmax {n}x{c}")


# ---------------------------------------------------------------- cross-entropy
def _ce_case(n, c, seed):
    """Integer logits in [-20, 20] with planted maxima of 50: row r ties j and j + d (d = 1, 33: different lanes; 64: the
    same lane) and labels the lower or the higher of the two; every sixth row is left as drawn."""
    z = _ints((n, c), -20, 20, seed).float()
    labels = _ints((n,), 0, c - 1, seed + 1)
    planted = 0
    for r in range(n):
        kind = (r + 1) % 6
        d = (0, 1, 1, 64, 64, 33)[kind]
        if d == 0 or c < 2:
            continue
        if d >= c:
            d = 1
        j = (7 * r) % (c - d)
        z[r, j] = z[r, j + d] = 50.0
        labels[r] = j if kind in (1, 3) else j + d
        planted += 1
    return z, labels, planted


def _argmax_lowest(z):
    ismax = z == z.max(1, keepdim=True).values
    cols = torch.arange(z.shape[1]).expand_as(z)
    return torch.where(ismax, cols, torch.full_like(cols, z.shape[1])).min(1).values


CE_CASES = [(n, c) for c in SM_C for n in CE_N]


@pytest.mark.parametrize("n,c", CE_CASES, ids=_ids(CE_CASES))
def test_exact_cross_entropy(n, c):
    from sykepic_hip import ops
    z, labels, planted = _ce_case(n, c, 100 * n + c)
    assert c < 2 or planted >= max(1, (5 * n) // 6 - 1)
    correct = int((_argmax_lowest(z) == labels).sum())
    assert c < 2 or n < 3 or 0 < correct < n        # both outcomes occur
    zd, ld = _dev(z), labels.cuda()
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz,), outside = _carve([(n, c)])
    ops.cross_entropy(zd, ld, stats, dz)
    _assert_untouched(flat, outside, "dz")
    s1 = stats.cpu().clone()
    assert float(s1[1]) == correct, f"correct rows: got {float(s1[1])}, expected {correct}"
    assert math.isfinite(float(s1[0])) and float(s1[0]) >= 0
    assert bool(torch.isfinite(dz).all())
    keep = flat.clone()
    ops.cross_entropy(zd, ld, stats, None)              # no gradient: same statistics, added to the first call's
    assert bool((flat == keep).all()), "a call without dz wrote the buffer of the earlier one"
    s2 = stats.cpu()
    assert float(s2[1]) == 2 * correct and float(s2[0]) == 2 * float(s1[0]), f"two calls: {s1.tolist()} then {s2.tolist()}"
    if c == 1:
        assert float(s1[0]) == 0.0 and not bool(dz.ne(0).any())


@pytest.mark.parametrize("n,c", [(33, 49), (17, 1000), (100, 130)], ids=lambda v: str(v))
def test_random_cross_entropy(n, c):
    from sykepic_hip import ops
    z = _normal((n, c), 8, 3.0)
    labels = _ints((n,), 0, c - 1, 9)
    p, e1, t, zs, s = _softmax_ref(z, 1.0)
    onehot = F.one_hot(labels, c).double()
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    dz = torch.full((n, c), float("nan"), dtype=torch.float32, device="cuda")
    ops.cross_entropy(_dev(z), labels.cuda(), stats, dz)
    _ratio(dz.cpu().double() * n, p - onehot, (2 * e1 + t) * p + 3 * EPS * (p - onehot).abs(), f"ce dz {n}x{c}")
    mx = zs.max(1, keepdim=True).values
    lse = (mx + torch.log(s)).squeeze(1)
    rows = lse - zs[torch.arange(n), labels]
    row_bound = (e1.squeeze(1) + t) + E_EXPF * torch.log(s).squeeze(1).abs() + EPS * (lse.abs() + rows.abs())
    bound = row_bound.sum() + (n / 16 + 17) * EPS * rows.abs().sum()
    _ratio(stats[:1], rows.sum().reshape(1), bound.reshape(1), f"ce loss {n}x{c}")
    assert float(stats[1]) == int((_argmax_lowest(z) == labels).sum())
