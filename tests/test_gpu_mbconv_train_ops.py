"""The MBConv training kernels (csrc/train_effnet.hip) one operator at a time, at the launch geometry production uses.

The kernels that train EfficientNet-B0...B7 and MobileNetV3 - depthwise forward / data gradient / weight gradient,
BatchNorm + SiLU / Hardswish / ReLU forward and backward, squeeze-excitation forward and backward, the 3x3 RGB stem and
its weight gradient - run here through the single-operator hooks `spk_op_dw_train`, `spk_op_bna_forward`,
`spk_op_bna_backward`, `spk_op_se_train_forward`, `spk_op_se_train_backward` and `spk_op_stem3_train` (sykepic_hip/ops.py),
which make the launches of a training step for ONE layer through the step's own dispatch functions.  The kernels are
linear in their data except for the activations, and the activation is a run-time argument that does not touch the
launch geometry, so there are two kinds of test.

1. EXACT (`test_exact_*`): integer-valued operands - activations and gradients from [-3, 3] (BatchNorm backward: up to
   |8|), weights from [-2, 2], all exact in bf16 - and a reference in integer arithmetic on the CPU (int64 sums; float64
   convolutions of integers, which are exact below 2^53).  Every fp32 partial sum is then an integer below 2^24 and
   every bf16 output an integer (or, BatchNorm backward, a half integer) of at most 8 significant bits, so the kernel's
   result must EQUAL the reference whatever the order of its sums: no tolerance.  Each test asserts both conditions on
   the reference first (sum of |terms| < 2^24; |value| <= 256 for bf16 outputs).  Asserted exactly:
   - depthwise: the raw forward output, dx (not accumulated: the eval path's kernel on the flipped window at stride 1;
     accumulated: dw_dgrad_px_kernel; pad 0: dw_fwd_kernel / dw_dgrad_kernel) and dw, for k 3 / 5 x stride 1 / 2 at
     sizes with w < k + 3, widths that are no multiple of 4, odd heights, both output parities at stride 2, channel
     tiles of every kind, and dw at 128 / 256 / 1024 items per block;
   - BatchNorm forward: the channel sums and sums of squares (read back as round(mean M), and from the running
     variance with momentum 1: requires sum x^2 < 2^23, asserted) at 64 ... 1024 rows per block; and, on data built to
     have mean 0 and variance 4 per channel with eps = 0 (invstd = 1/2 exactly, gamma 2: scale 1, shift = beta), st
     itself, out = act(raw + beta) * rowscale + res for act none / ReLU with rowscale 0 / 2, and the pooled chunk sums
     of `bna_apply_pool`;
   - BatchNorm backward with act none, mean 0, invstd 1, scale 1, shift 0 on data built so that mean(dz) and
     mean(dz xhat) are small integers: dgamma, dbeta, dy = gamma (g - k0 - raw k1) with gamma a power of two, g_res in
     both forms; with rowscale 0 / 2 per image dgamma / dbeta (dy is then only bounded);
   - `pool_rows(g, a)` (the per-chunk sums of the squeeze-excitation backward) for HW 1 ... 3137;
   - `se_wgrad` on integer du2 / h1 / du1 / pooled for every SJ 12 ... 16 and batches of 1 / 5 / 33;
   - the derivative on its kinks, planted (raw in {-3, 0, 3}, scale 1, shift 0): equal to torch autograd's own value
     there.  FOUND HERE: the kernels took Hardswish' on the closed interval [-3, 3] (-1/2 at -3, 3/2 at 3, the values of
     older torch releases); torch 2.10's hardswish_backward uses the open interval (0 at -3, 1 at 3).  `hswish_grad`
     (csrc/train_effnet.hip) now does the same; ReLU' = 0 at 0 and Hardsigmoid' = 0 at +-3 already agreed;
   - zeros in the pad channels (c >= c_log) of every output that has them.
2. BOUNDED (`test_random_*`): normal operands against a float64 reference built from the same rounded operands (each
   stage of a chain from the operands the kernel itself left for it, so a stage is judged on its own).  With A the
   float64 sum of the absolute values of the terms of the final expression:
   - bf16 outputs |got - ref| <= 2^-8 |ref| + 2^-16 A, fp32 outputs 2^-20 |ref| + 2^-16 A;
   - batch mean within 2^-12 of the channel's rms, invstd within 2^-12 relative;
   - fp32 reductions over rows (dgamma, dbeta, dw of the stem): 2^-14 sum |terms| - derived: the longest sequential
     fp32 chain in these kernels is about 1056 additions (8192 items / 32 rows in flight x 4 pixels, plus 32), each
     at most 2^-24 of the running sum of |terms|: 1056 x 2^-24 < 2^-13.9.
   Elements whose float64 pre-activation lies within 2^-16 (|raw scale| + |shift|) of a kink (ReLU: 0; Hardswish': +-3)
   are left out of the element-wise checks (their terms go into the bounds of the sums instead); at most 0.1 % may be.
   The bounds are derived, none is taken from what the kernels give; none has been re-measured or widened.

Coverage of the launch geometry is asserted without a GPU by tests/test_host_mbconv_geometry.py, which feeds the case
lists below through `spk_op_mbconv_geometry` (the launchers' own helpers).

Not covered / unreachable:
- the grid-stride clamp of `grid_of` (65535 x 16 blocks) needs tensors above 2 G elements;
- `stem3_wgrad_kernel` (the variant that is not the register-tile one) is unreachable whenever cout % 4 == 0, which
  holds for every stem of `arch.build_graph`; no case here reaches it;
- `dw_fwd_kernel` and `dw_dgrad_kernel` only run when pad != (k-1)/2, which no network of `arch.build_graph` has; they
  are run here through the hook at pad 0 (all four (k, stride) instantiations of each);
- `sd_rowscale_kernel` (the stochastic-depth draw) and `slab_reduce_sub_kernel` have no hook of their own.

Wall time of this file on an MI355X: 11 s for its 232 tests; the slowest are test_exact_dw_train[2x9x7x64x40x3x1x1]
(1.4 s: the first launch of the process), test_exact_dw_wgrad_rows_per_block[2x724x724x64x40x3x1x1] (1.3 s) and
test_exact_bna_backward[4x262160x64x40] (1.1 s), every other one under 0.6 s.  The 67 M-element cases
(BNA_BIG_CASES[-1], DW_BIG_CASES[-1]) run once each, on integer data only.
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_SILU, ACT_HSWISH = 0, 1, 2, 3

# ---------------------------------------------------------------- cases (read by tests/test_host_mbconv_geometry.py)
# depthwise: (n, h, w, C, c_log, k, stride, pad); every case runs y, dx (accumulate 0 and 1) and dw
DW_SHAPES = [(2, 9, 7), (3, 13, 10), (1, 5, 5)]
DW_CHANNELS = [(64, 40), (192, 184)]
DW_CASES = [(n, h, w, C, cl, k, s, (k - 1) // 2)
            for (n, h, w) in DW_SHAPES for (C, cl) in DW_CHANNELS for k in (3, 5) for s in (1, 2)]
DW_CASES += [(2, 6, 6, 64, 40, 3, 2, 1), (2, 6, 6, 64, 40, 5, 2, 2)]           # ho * 2 != h + 1: both parity classes
DW_CASES += [(1, 5, 5, C, cl, k, s, (k - 1) // 2)                               # two tiles, even tiles, uneven tiles
             for (C, cl) in ((320, 300), (512, 480), (1152, 1152)) for (k, s) in ((3, 1), (5, 2))]
DW_CASES += [(2, 9, 7, 64, 40, 3, 1, 0), (2, 9, 7, 64, 40, 3, 2, 0),           # pad 0: dw_fwd_kernel, dw_dgrad_kernel
             (3, 13, 10, 192, 184, 5, 1, 0), (3, 13, 10, 192, 184, 5, 2, 0)]
# weight gradient only, int8 operands: 128, 256 and 1024 items per block
DW_BIG_CASES = [(2, 181, 363, 64, 40, 3, 1, 1), (2, 182, 724, 64, 64, 3, 1, 1), (2, 724, 724, 64, 40, 3, 1, 1)]

# BatchNorm + activation: (n, HW, C, c_log), M = n * HW rows
BNA_SMALL_CASES = [(n, hw, C, cl) for (n, hw) in ((2, 49), (3, 197))
                   for (C, cl) in ((64, 40), (192, 184), (320, 320), (512, 480), (1152, 1152))]
# exact only: 128, 256, 512 and 1024 rows per block; HW divides no rows-per-block
BNA_BIG_CASES = [(8, 16369, 64, 40), (16, 16375, 64, 64), (32, 16375, 64, 64), (4, 262160, 64, 40)]

# pooling (pool_part of bna_apply_pool, pool_rows(g, a)): (n, HW, C, c_log)
POOL_CASES = [(5, 1, 64, 40), (1, 49, 192, 184), (5, 195, 64, 40), (5, 196, 320, 300), (1, 197, 1152, 1152),
              (33, 197, 128, 96), (5, 3136, 64, 40), (1, 3137, 192, 184), (1, 3137, 1152, 1152), (5, 49, 3840, 3840),
              (5, 49, 512, 480), (1, 196, 1024, 960)]
# squeeze-excitation, forward and backward on random data: (n, HW, C, Cl, S)
SE_CASES = [(1, 49, 64, 40, 10), (5, 197, 128, 96, 4), (5, 49, 512, 480, 120), (1, 196, 1024, 960, 240),
            (5, 1, 3840, 3840, 160), (33, 49, 1152, 1152, 48), (5, 3137, 64, 40, 10), (33, 1, 1024, 960, 240)]
# se_wgrad on integer vectors: (n, C, Cl, S)
SE_WGRAD_CASES = [(n, C, cl, S) for n in (1, 5, 33)
                  for (C, cl, S) in ((64, 40, 10), (128, 96, 4), (512, 480, 120), (1024, 960, 240), (3840, 3840, 160),
                                     (1152, 1152, 48), (64, 64, 200), (128, 100, 216), (64, 40, 256), (64, 64, 192))]
# stem: (n, h, w, cin, cout)
STEM_CASES = [(2, 9, 10, 3, 32), (1, 33, 18, 3, 40), (3, 64, 64, 1, 16), (2, 7, 8, 3, 64)]

TWO24 = 2 ** 24


# ---------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed), dtype=torch.int8)


def _zero_pad(t, c_log):
    if c_log < t.shape[-1]:
        t[..., c_log:] = 0
    return t


def _dev(t, dtype=torch.bfloat16):
    return t.cuda().to(dtype).contiguous()


def _assert_equal(got, exp, what):
    """got: device tensor; exp: CPU tensor of exactly representable values.  Equal as numbers (-0 == +0), NaN fails."""
    g = got.float()
    e = exp.to(got.device).float().reshape(g.shape)
    bad = ~(g == e)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[0].tolist()
        t = tuple(idx)
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements differ; first at {idx}: got {float(g[t])}, "
                             f"expected {float(e[t])}")


def _assert_pad_zero(got, c_log, what):
    if c_log < got.shape[-1]:
        assert not bool(got[..., c_log:].float().ne(0).any()), f"{what}: pad channels are not zero"


def _check_close(got, ref, A, what, rel, skip=None, extra=None):
    """|got - ref| <= rel |ref| + 2^-16 A (+ extra), float64 on the CPU; `skip`: elements left out (kinks)."""
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (unwritten elements?)"
    bound = rel * ref.abs() + 2.0 ** -16 * A
    if extra is not None:
        bound = bound + extra
    over = (got - ref).abs() - bound
    if skip is not None:
        over = torch.where(skip, torch.full_like(over, -1.0), over)
    worst = float(over.max())
    if worst > 0:
        i = int(over.argmax())
        raise AssertionError(f"{what}: element {i} off by {float((got - ref).abs().flatten()[i]):.4e}, bound "
                             f"{float(bound.flatten()[i]):.4e} (ref {float(ref.flatten()[i]):.5e})")


BF16, FP32 = 2.0 ** -8, 2.0 ** -20


# ---------------------------------------------------------------- depthwise, exact
def _dw_ref_small(x, dy, w, k, stride, pad, acc0):
    """float64 autograd on integer operands (exact): x [n,h,w,C], dy [n,ho,wo,C], w [C,k*k] (zeros in the pad rows)."""
    C = x.shape[-1]

    def run(xv, wv, gv):
        xt = xv.permute(0, 3, 1, 2).double().requires_grad_(True)
        wt = wv.reshape(C, 1, k, k).double().requires_grad_(True)
        y = F.conv2d(xt, wt, None, stride, pad, 1, C)
        y.backward(gv.permute(0, 3, 1, 2).double())
        return y.detach().permute(0, 2, 3, 1), xt.grad.permute(0, 2, 3, 1), wt.grad.reshape(C, k * k)

    y, dx, dw = run(x, w, dy)
    ya, dxa, dwa = run(x.abs(), w.abs(), dy.abs())
    assert float(ya.max()) < TWO24 and float(dxa.max()) + 3 < TWO24 and float(dwa.max()) < TWO24
    assert float(y.abs().max()) <= 256 and float(dx.abs().max()) + 3 <= 256
    return y, dx, dx + acc0.double(), dw


def _dw_ref_dw_int(x8, dy8, k, stride, pad):
    """dw [C, k*k] int64 from int8 operands by shifted slices (products of magnitude <= 9 stay in int8)."""
    n, h, w, C = x8.shape
    _, ho, wo, _ = dy8.shape
    dw = torch.zeros((C, k * k), dtype=torch.int64)
    for kh in range(k):
        for kw in range(k):
            oh0 = max(0, -((kh - pad) // stride))          # first oh with oh * stride + kh - pad >= 0
            ow0 = max(0, -((kw - pad) // stride))
            oh1 = min(ho, (h - 1 - kh + pad) // stride + 1)
            ow1 = min(wo, (w - 1 - kw + pad) // stride + 1)
            if oh1 <= oh0 or ow1 <= ow0:
                continue
            ih0, iw0 = oh0 * stride + kh - pad, ow0 * stride + kw - pad
            xs = x8[:, ih0:ih0 + (oh1 - oh0 - 1) * stride + 1:stride, iw0:iw0 + (ow1 - ow0 - 1) * stride + 1:stride]
            dw[:, kh * k + kw] = (xs * dy8[:, oh0:oh1, ow0:ow1]).sum(dim=(0, 1, 2), dtype=torch.int64)
    return dw


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_dw_train(case):
    from sykepic_hip import ops
    n, h, w, C, cl, k, stride, pad = case
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    seed = hash(case) % 10000
    x = _zero_pad(_ints((n, h, w, C), -3, 3, seed), cl)
    dy = _zero_pad(_ints((n, ho, wo, C), -3, 3, seed + 1), cl)
    acc0 = _zero_pad(_ints((n, h, w, C), -3, 3, seed + 2), cl)
    wgt = torch.zeros((C, k * k), dtype=torch.int8)
    wgt[:cl] = _ints((cl, k * k), -2, 2, seed + 3)
    y_ref, dx_ref, dxa_ref, dw_ref = _dw_ref_small(x, dy, wgt, k, stride, pad, acc0)
    assert torch.equal(dw_ref.long(), _dw_ref_dw_int(x, dy, k, stride, pad)), "the two references disagree"
    xd, dyd, wd = _dev(x), _dev(dy), _dev(wgt[:cl], torch.float32)
    r = ops.dw_train(xd, wd, cl, k, stride, pad, dy=dyd, want_y=True, want_dx=True, want_dw=True)
    _assert_equal(r["y"], y_ref, "y")
    _assert_equal(r["dx"], dx_ref, "dx (accumulate 0)")
    _assert_equal(r["dw"], dw_ref[:cl], "dw")
    ra = ops.dw_train(xd, wd, cl, k, stride, pad, dy=dyd, want_y=False, accumulate_into=_dev(acc0))
    _assert_equal(ra["dx"], dxa_ref, "dx (accumulate 1)")
    for name, t in (("y", r["y"]), ("dx", r["dx"]), ("dx+", ra["dx"])):
        _assert_pad_zero(t, cl, name)


@pytest.mark.parametrize("case", DW_BIG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_dw_wgrad_rows_per_block(case):
    from sykepic_hip import ops
    n, h, w, C, cl, k, stride, pad = case
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x = _zero_pad(_ints((n, h, w, C), -3, 3, 11), cl)
    dy = _zero_pad(_ints((n, ho, wo, C), -3, 3, 12), cl)
    assert 9 * n * ho * wo < TWO24          # sum of |terms| <= 9 per output pixel
    dw_ref = _dw_ref_dw_int(x, dy, k, stride, pad)
    r = ops.dw_train(_dev(x), torch.zeros((cl, k * k), device="cuda"), cl, k, stride, pad, dy=_dev(dy), want_y=False,
                     want_dw=True)
    _assert_equal(r["dw"], dw_ref[:cl], "dw")


def test_random_dw_weights_are_rounded_to_bf16():
    """The packed window holds bf16(w): the forward output and dx follow the rounded weights, dw does not see them."""
    from sykepic_hip import ops
    n, h, w, C, cl, k, stride = 2, 9, 7, 64, 40, 3, 1
    x = _zero_pad(_ints((n, h, w, C), -3, 3, 5), cl)
    wgt = torch.zeros((C, k * k))
    wgt[:cl] = torch.randn((cl, k * k), generator=_gen(6))
    assert not torch.equal(wgt.bfloat16().float(), wgt)
    wr = wgt.bfloat16().double()
    xt = x.permute(0, 3, 1, 2).double()
    y_ref = F.conv2d(xt, wr.reshape(C, 1, k, k), None, stride, 1, 1, C).permute(0, 2, 3, 1)
    A = F.conv2d(xt.abs(), wr.abs().reshape(C, 1, k, k), None, stride, 1, 1, C).permute(0, 2, 3, 1)
    r = ops.dw_train(_dev(x), _dev(wgt[:cl], torch.float32), cl, k, stride, want_y=True)
    _check_close(r["y"], y_ref, A, "y", BF16)
    dx_ref = F.conv_transpose2d(xt, wr.reshape(C, 1, k, k), None, stride, 1, 0, C).permute(0, 2, 3, 1)
    r = ops.dw_train(_dev(x), _dev(wgt[:cl], torch.float32), cl, k, stride, dy=_dev(x), want_y=False, want_dx=True)
    A = F.conv_transpose2d(xt.abs(), wr.abs().reshape(C, 1, k, k), None, stride, 1, 0, C).permute(0, 2, 3, 1)
    _check_close(r["dx"], dx_ref, A, "dx", BF16)


# ---------------------------------------------------------------- BatchNorm + activation, exact
def _structured(M, C, seed):
    """raw, g0 [M, C] int8 with, per channel: sum raw = 0, sum raw^2 = 4 M, sum g0 = 0, sum g0 raw = 0.
    Rows come in quads raw = (v, v, -v, -v), g0 = (p, -p, q, -q) with v = 2, or v = 1 / 3 in the ratio 5 : 3; what is
    left of M takes (3, -3, 1, -1, 0) and (2, -2) with g0 = 0; one random row order, rolled and sign-flipped per channel."""
    assert M >= 5 or M % 2 == 0
    g = _gen(seed)
    raw, g0 = [], []
    left = M
    if M % 4 in (1, 3):
        raw += [3, -3, 1, -1, 0]
        g0 += [0] * 5
        left -= 5
    if left % 4 == 2:
        raw += [2, -2]
        g0 += [0, 0]
        left -= 2
    Q = left // 4
    nb = (Q // 8 + 1) // 2
    v = torch.cat([torch.tensor([1, 1, 1, 1, 1, 3, 3, 3]).repeat(nb), torch.full((Q - 8 * nb,), 2)]).long()
    p = torch.randint(-3, 4, (Q,), generator=g)
    q = torch.randint(-3, 4, (Q,), generator=g)
    raw = torch.cat([torch.tensor(raw, dtype=torch.long), torch.stack([v, v, -v, -v], 1).flatten()]).to(torch.int8)
    g0 = torch.cat([torch.tensor(g0, dtype=torch.long), torch.stack([p, -p, q, -q], 1).flatten()]).to(torch.int8)
    perm = torch.randperm(M, generator=g)
    raw, g0 = raw[perm], g0[perm]
    offs = torch.randint(0, M, (C,), generator=g)
    sign = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).to(torch.int8)
    raw2 = torch.cat([raw, raw]).unfold(0, M, 1)[offs] * sign[:, None]        # [C, M]
    g02 = torch.cat([g0, g0]).unfold(0, M, 1)[offs]
    return raw2.t().contiguous(), g02.t().contiguous()


def _chunk_sums(t, chunks):
    """[n, HW, C] integer tensor -> [n, chunks, C] int64 sums over ceil(HW / chunks) rows each."""
    n, hw, C = t.shape
    rows = (hw + chunks - 1) // chunks
    out = torch.zeros((n, chunks, C), dtype=torch.int64)
    for q in range(chunks):
        if q * rows < hw:
            out[:, q] = t[:, q * rows:min(hw, (q + 1) * rows)].sum(dim=1, dtype=torch.int64)
    return out


@pytest.mark.parametrize("case", BNA_SMALL_CASES + BNA_BIG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_bna_forward_sums(case):
    """Channel sums and sums of squares of random integers, read back from the batch mean and the running variance."""
    from sykepic_hip import ops
    n, hw, C, cl = case
    M = n * hw
    x = _zero_pad(_ints((n, hw, C), -3, 3, 21), cl)
    s1 = x.sum(dim=(0, 1), dtype=torch.int64)
    s2 = (x * x).sum(dim=(0, 1), dtype=torch.int64)
    assert int(s2.max()) < 2 ** 23        # round(fl32(s / M) * M) == s needs |s| 2^-24 < 1/2 (and < 2^24 for the sums)
    rm = torch.zeros(cl, device="cuda")
    rv = torch.zeros(cl, device="cuda")
    ones = torch.ones(cl, device="cuda")
    r = ops.bna_forward(_dev(x), ones, torch.zeros(cl, device="cuda"), rm, rv, act=ACT_NONE, eps=1e-5, momentum=1.0)
    st = r["st"].cpu().double()
    assert torch.equal(torch.round(st[0, :cl] * M).long(), s1[:cl]), "sum x (from the batch mean)"
    assert torch.equal(torch.round(rm.cpu().double() * M).long(), s1[:cl]), "sum x (from the running mean)"
    mean = s1[:cl].double() / M
    got_s2 = torch.round((rv.cpu().double() * (M - 1) / M + mean * mean) * M).long()
    assert torch.equal(got_s2, s2[:cl]), "sum x^2 (from the running variance)"
    var = s2[:cl].double() / M - mean * mean
    inv = 1.0 / torch.sqrt(var + 1e-5)
    assert float(((st[1, :cl] - inv).abs() / inv).max()) <= 2.0 ** -12, "invstd"
    assert not bool(st[:, cl:].ne(0).any()), "st: pad channels are not zero"


@pytest.mark.parametrize("case", BNA_SMALL_CASES + BNA_BIG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_bna_forward_apply_and_pool(case):
    """mean 0, variance 4, eps 0, gamma 2: scale 1, shift = beta; out = act(raw + beta) * rowscale + res exactly."""
    from sykepic_hip import ops
    n, hw, C, cl = case
    M = n * hw
    raw, _ = _structured(M, C, 31)
    raw = _zero_pad(raw, cl).reshape(n, hw, C)
    flat = raw.reshape(M, C)
    assert int(flat.sum(0, dtype=torch.int64).abs().max()) == 0
    assert torch.equal((flat * flat).sum(0, dtype=torch.int64)[:cl], torch.full((cl,), 4 * M))
    beta = torch.randint(-2, 3, (cl,), generator=_gen(32)).to(torch.int8)
    res = _zero_pad(_ints((n, hw, C), -3, 3, 33), cl)
    rs = torch.randint(0, 2, (n,), generator=_gen(34)).to(torch.int8) * 2
    betaC = torch.zeros(C, dtype=torch.int8)
    betaC[:cl] = beta
    gamma = torch.full((cl,), 2.0, device="cuda")
    rawd, betad = _dev(raw), _dev(beta, torch.float32)
    st_ref = torch.zeros((4, C))
    st_ref[1, :cl], st_ref[2, :cl], st_ref[3, :cl] = 0.5, 1.0, beta.float()
    # act none, shortcut and per-image factor
    rm, rv = torch.zeros(cl, device="cuda"), torch.ones(cl, device="cuda")
    r = ops.bna_forward(rawd, gamma, betad, rm, rv, act=ACT_NONE, res=_dev(res), rowscale=_dev(rs, torch.float32),
                        eps=0.0, momentum=0.5)
    _assert_equal(r["st"], st_ref, "st")
    out_ref = (raw + betaC) * rs[:, None, None] + res            # int8: |.| <= 13
    _assert_equal(r["out"], out_ref, "out (none, res, rowscale)")
    _assert_equal(rm, torch.zeros(cl), "running mean")
    rv_ref = 0.5 + 0.5 * (4.0 * M / (M - 1))
    assert float((rv.cpu().double() - rv_ref).abs().max()) <= 2.0 ** -21 * rv_ref, "running variance"
    # ReLU and the squeeze of the layer behind
    rm, rv = torch.zeros(cl, device="cuda"), torch.ones(cl, device="cuda")
    r = ops.bna_forward(rawd, gamma, betad, rm, rv, act=ACT_RELU, pool=True, eps=0.0, momentum=0.5)
    out_ref = (raw + betaC).clamp_(min=0)
    _assert_equal(r["st"], st_ref, "st")
    _assert_equal(r["out"], out_ref, "out (ReLU, pool)")
    part_ref = _chunk_sums(out_ref, r["pool_part"].shape[1])
    assert int(part_ref.max()) < TWO24
    _assert_equal(r["pool_part"], part_ref, "pool_part")


def _bna_bwd_exact_operands(n, hw, C, cl, seed):
    M = n * hw
    raw, g0 = _structured(M, C, seed)
    g = _gen(seed + 1)
    a = torch.randint(-2, 3, (C,), generator=g).to(torch.int8)
    c = torch.randint(-1, 2, (C,), generator=g).to(torch.int8)
    gam = 2.0 ** torch.randint(-1, 3, (cl,), generator=g).float()
    gg = g0 + a[None, :] + c[None, :] * raw                       # |g| <= 8
    raw, gg = _zero_pad(raw, cl), _zero_pad(gg, cl)
    st = torch.zeros((4, C))
    st[1, :cl], st[2, :cl] = 1.0, 1.0
    return raw.reshape(n, hw, C), gg.reshape(n, hw, C), a, c, gam, st


@pytest.mark.parametrize("case", BNA_SMALL_CASES + BNA_BIG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_bna_backward(case):
    from sykepic_hip import ops
    n, hw, C, cl = case
    M = n * hw
    raw, g, a, c, gam, st = _bna_bwd_exact_operands(n, hw, C, cl, 41)
    rf, gf = raw.reshape(M, C), g.reshape(M, C)
    s1 = gf.sum(0, dtype=torch.int64)
    s2 = (gf.short() * rf.short()).sum(0, dtype=torch.int64)
    assert torch.equal(s1[:cl], a[:cl].long() * M) and torch.equal(s2[:cl], 4 * c[:cl].long() * M)
    assert int((gf.short() * rf.short()).abs_().sum(0, dtype=torch.int64).max()) < TWO24
    gamC = torch.zeros(C)
    gamC[:cl] = gam
    dy_ref = (g.short() - a.short() - raw.short() * (4 * c.short())).float() * gamC     # half integers, |.| <= 17 * 4
    assert float(dy_ref.abs().max()) <= 256
    gres0 = _zero_pad(_ints((n, hw, C), -3, 3, 43), cl)
    gd, rawd, std, gamd = _dev(g), _dev(raw), st.cuda(), gam.cuda()
    r = ops.bna_backward(gd, rawd, std, gamd, act=ACT_NONE, want_res=True)
    _assert_equal(r["dbeta"], s1[:cl], "dbeta")
    _assert_equal(r["dgamma"], s2[:cl], "dgamma")
    _assert_equal(r["dy"], dy_ref, "dy")
    _assert_equal(r["g_res"], g, "g_res (stored)")
    r = ops.bna_backward(gd, rawd, std, gamd, act=ACT_NONE, g_res=_dev(gres0))
    _assert_equal(r["dy"], dy_ref, "dy")
    _assert_equal(r["g_res"], gres0 + g, "g_res (accumulated)")
    _assert_pad_zero(r["dy"], cl, "dy")


@pytest.mark.parametrize("case", [(2, 49, 192, 184), (3, 197, 1152, 1152), (8, 16369, 64, 40)],
                         ids=lambda c: "x".join(map(str, c)))
def test_exact_bna_backward_rowscale_sums(case):
    """A per-image factor of 0 / 2 (HW divides no rows-per-block): dgamma / dbeta are still integer sums."""
    from sykepic_hip import ops
    n, hw, C, cl = case
    raw = _zero_pad(_ints((n, hw, C), -3, 3, 51), cl)
    g = _zero_pad(_ints((n, hw, C), -3, 3, 52), cl)
    rs = (torch.arange(n) % 2 * 2).to(torch.int8)
    if n > 2:
        rs[-1] = 2
    dz = g * rs[:, None, None]
    s1 = dz.sum(dim=(0, 1), dtype=torch.int64)
    s2 = (dz * raw).sum(dim=(0, 1), dtype=torch.int64)
    assert 18 * n * hw < TWO24
    st = torch.zeros((4, C))
    st[1, :cl], st[2, :cl] = 1.0, 1.0
    r = ops.bna_backward(_dev(g), _dev(raw), st.cuda(), torch.ones(cl, device="cuda"), act=ACT_NONE,
                         rowscale=_dev(rs, torch.float32))
    _assert_equal(r["dbeta"], s1[:cl], "dbeta")
    _assert_equal(r["dgamma"], s2[:cl], "dgamma")
    M = n * hw
    k0, k1 = s1.double() / M, s2.double() / M
    k0[cl:], k1[cl:] = 0, 0
    dy_ref = dz.double() - k0 - raw.double() * k1
    A = dz.double().abs() + k0.abs() + (raw.double() * k1).abs()
    _check_close(r["dy"], dy_ref, A, "dy", BF16)


def test_exact_activation_derivative_on_its_kinks():
    """raw in {-3, 0, 3} with scale 1, shift 0: the derivative there is torch autograd's own value (torch 2.10:
    Hardswish' = 0 at -3, 1/2 at 0, 1 at 3 - the open interval; ReLU' = 0 at 0).  Rows are quads raw = (v, v, -v, -v),
    g = (p, -p, q, -q): sum dz = sum dz xhat = 0 exactly, so dy = g act'(raw) and dgamma = dbeta = 0."""
    from sykepic_hip import ops
    C, Q = 64, 24
    g = _gen(61)
    v = torch.randint(0, 2, (Q, C), generator=g) * 3
    p = torch.randint(-3, 4, (Q, C), generator=g)
    q = torch.randint(-3, 4, (Q, C), generator=g)
    raw = torch.stack([v, v, -v, -v], 1).reshape(1, 4 * Q, C).float()
    gg = torch.stack([p, -p, q, -q], 1).reshape(1, 4 * Q, C).float()
    st = torch.zeros((4, C))
    st[1], st[2] = 1.0, 1.0
    for act, fn in ((ACT_HSWISH, F.hardswish), (ACT_RELU, F.relu)):
        z = raw.clone().requires_grad_(True)
        fn(z).backward(gg)
        r = ops.bna_backward(_dev(gg), _dev(raw), st.cuda(), torch.ones(C, device="cuda"), act=act)
        _assert_equal(r["dy"], z.grad, f"dy (act {act})")
        _assert_equal(r["dbeta"], torch.zeros(C), "dbeta")
        _assert_equal(r["dgamma"], torch.zeros(C), "dgamma")


# ---------------------------------------------------------------- BatchNorm + activation, bounded
def _act64(z, act):
    if act == ACT_RELU:
        return z.clamp(min=0)
    if act == ACT_SILU:
        return z / (1 + torch.exp(-z))
    if act == ACT_HSWISH:
        return z * (z + 3).clamp(0, 6) / 6
    return z


def _act_grad64(z, act):
    if act == ACT_RELU:
        return (z > 0).double()
    if act == ACT_SILU:
        s = 1 / (1 + torch.exp(-z))
        return s * (1 + z * (1 - s))
    if act == ACT_HSWISH:
        return torch.where(z < -3, torch.zeros_like(z), torch.where(z <= 3, z / 3 + 0.5, torch.ones_like(z)))
    return torch.ones_like(z)


KINKS = {ACT_NONE: (), ACT_RELU: (0.0,), ACT_SILU: (), ACT_HSWISH: (-3.0, 3.0)}


def _near_kink(z, width, act, c_log):
    """Elements of the logical channels within `width` of a kink (the pad channels hold zeros and take no part)."""
    near = torch.zeros_like(z, dtype=torch.bool)
    for kk in KINKS[act]:
        near |= (z - kk).abs() <= width
    near[..., c_log:] = False
    assert float(near[..., :c_log].double().mean()) <= 1e-3, "more than 0.1 % of the elements lie on a kink"
    return near


@pytest.mark.parametrize("variant", ["plain", "res_rowscale"])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU, ACT_HSWISH])
@pytest.mark.parametrize("case", BNA_SMALL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_bna_forward_backward(case, act, variant):
    from sykepic_hip import ops
    n, hw, C, cl = case
    M = n * hw
    gn = _gen(71 + act)
    mk = lambda scale, shift=0.0: _zero_pad((torch.randn((n, hw, C), generator=gn) * scale + shift).bfloat16(), cl)  # noqa: E731
    raw, g = mk(1.5, 0.3), mk(1.0)
    full = variant == "res_rowscale"
    res = mk(1.0) if full else None
    gres0 = mk(1.0) if full else None
    rs = torch.tensor([0.0, 1.25, 1.25][:n]) if full else None
    gamma = torch.rand(cl, generator=gn) + 0.5
    beta = torch.randn(cl, generator=gn) * 0.5
    rm0, rv0 = torch.randn(cl, generator=gn), torch.rand(cl, generator=gn) + 0.5
    rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
    eps, mom = 1e-3, 0.1
    rawd = raw.cuda()
    r = ops.bna_forward(rawd, gamma.cuda(), beta.cuda(), rm, rv, act=act, res=res.cuda() if full else None,
                        rowscale=rs.cuda() if full else None, eps=eps, momentum=mom)
    # statistics
    x = raw.double().reshape(M, C)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    inv = 1 / torch.sqrt(var + eps)
    st = r["st"].cpu().double()
    rms = torch.sqrt((x * x).mean(0))
    assert bool(((st[0] - mean).abs()[:cl] <= 2.0 ** -12 * rms[:cl]).all()), "batch mean"
    assert bool((((st[1] - inv).abs() / inv)[:cl] <= 2.0 ** -12).all()), "invstd"
    assert not bool(st[:, cl:].ne(0).any()), "st: pad channels"
    sc_ref = gamma.double() * st[1, :cl]
    sh_ref = beta.double() - st[0, :cl] * sc_ref
    _check_close(st[2, :cl], sc_ref, sc_ref.abs(), "scale", FP32)
    _check_close(st[3, :cl], sh_ref, beta.double().abs() + (st[0, :cl] * sc_ref).abs(), "shift", FP32)
    unb = var * M / (M - 1)
    # (the batch statistics inside carry their own bounds: 2^-12 rms for the mean, twice 2^-12 relative for the variance)
    _check_close(rm, (1 - mom) * rm0.double() + mom * mean[:cl], rm0.double().abs() + rms[:cl], "running mean", FP32,
                 extra=mom * 2.0 ** -12 * rms[:cl])
    _check_close(rv, (1 - mom) * rv0.double() + mom * unb[:cl], rv0.double() + unb[:cl], "running var", FP32,
                 extra=mom * 2.0 ** -11 * (unb + mean * mean)[:cl])
    # apply: from the kernel's own scale / shift
    sc, sh = st[2], st[3]
    xr = raw.double()
    z = xr * sc + sh
    zA = (xr * sc).abs() + sh.abs()
    rsv = rs.double()[:, None, None] if full else 1.0
    out_ref = _act64(z, act) * rsv + (res.double() if full else 0.0)
    A = zA * (rsv if full else 1.0) + (res.double().abs() if full else 0.0)
    _check_close(r["out"], out_ref, A, "out", BF16)      # (the activations are continuous: nothing to leave out)
    _assert_pad_zero(r["out"], cl, "out")
    # backward
    b = ops.bna_backward(g.cuda(), rawd, r["st"], gamma.cuda(), act=act, rowscale=rs.cuda() if full else None,
                         g_res=gres0.cuda() if full else None, want_res=True)
    near = _near_kink(z, 2.0 ** -16 * zA, act, cl)
    gz = g.double() * rsv
    dz = gz * _act_grad64(z, act)
    xh = (xr - st[0]) * st[1]
    unsure = torch.where(near, gz.abs() * 1.5, torch.zeros_like(gz))          # a derivative jumps by at most 1.5
    s1, s2 = dz.reshape(M, C).sum(0), (dz * xh).reshape(M, C).sum(0)
    t1 = 2.0 ** -14 * dz.abs().reshape(M, C).sum(0) + unsure.reshape(M, C).sum(0)
    t2 = 2.0 ** -14 * (dz * xh).abs().reshape(M, C).sum(0) + (unsure * xh.abs()).reshape(M, C).sum(0)
    db, dg = b["dbeta"].cpu().double(), b["dgamma"].cpu().double()
    assert bool(((db - s1[:cl]).abs() <= t1[:cl]).all()), f"dbeta: worst {(db - s1[:cl]).abs().max():.3e}"
    assert bool(((dg - s2[:cl]).abs() <= t2[:cl]).all()), f"dgamma: worst {(dg - s2[:cl]).abs().max():.3e}"
    k2 = torch.zeros(C, dtype=torch.float64)
    k2[:cl] = gamma.double() * st[1, :cl]
    k0, k1 = s1 / M, s2 / M
    dy_ref = k2 * (dz - k0 - xh * k1)
    Ady = k2.abs() * (dz.abs() + k0.abs() + (xh * k1).abs())
    extra = k2.abs() * (t1 / M + xh.abs() * t2 / M)
    _check_close(b["dy"], dy_ref, Ady, "dy", BF16, skip=near, extra=extra)
    _assert_pad_zero(b["dy"], cl, "dy")
    gres_ref = (gres0.float() + g.float()).bfloat16() if full else g
    _assert_equal(b["g_res"], gres_ref.float(), "g_res")


# ---------------------------------------------------------------- pooling and squeeze-excitation
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_pool_rows(case):
    """pool_rows(g, a): the per-chunk sums over HW of g * a, through the backward hook (gates of a zero layer)."""
    from sykepic_hip import ops
    n, hw, C, cl = case
    S = 8
    a = _zero_pad(_ints((n, hw, C), -3, 3, 81), cl)
    g = _zero_pad(_ints((n, hw, C), -3, 3, 82), cl)
    chunks = ops.mbconv_geometry(2, c=C, hw=hw)[1]
    ref = _chunk_sums(a * g, chunks)
    assert int(_chunk_sums((a * g).abs_(), chunks).max()) < TWO24
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    saved = {"gate": torch.full((n, C), 0.5, device="cuda"), "u1": z(n, S), "h1": z(n, S), "pooled": z(n, C)}
    r = ops.se_train_backward(_dev(g), _dev(a), saved, z(S, cl), z(cl, S), gate_kind=0)
    _assert_equal(r["pool_part"], ref, "pool_part")
    # W1 = W2 = 0: du1 = 0, dpool = 0, da = g * gate = g / 2 exactly
    _assert_equal(r["da"], g.float() * 0.5, "da")
    dg = ref.sum(1)
    du2_ref = torch.zeros((n, C), dtype=torch.float64)
    du2_ref[:, :cl] = dg[:, :cl].double() * 0.25          # s (1 - s) at s = 1/2
    _assert_equal(r["du2"], du2_ref, "du2")


@pytest.mark.parametrize("gate_kind", [0, 1])
@pytest.mark.parametrize("case", SE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_se_forward_backward(case, gate_kind):
    from sykepic_hip import ops
    n, hw, C, cl, S = case
    gn = _gen(91 + gate_kind)
    mk = lambda: _zero_pad(torch.randn((n, hw, C), generator=gn).bfloat16(), cl)   # noqa: E731
    a, g = mk(), mk()
    if hw > 1:
        a = _zero_pad((a.float() + 0.5).bfloat16(), cl)       # a pooled mean that is not noise around zero
    w1 = torch.randn((S, cl), generator=gn) / math.sqrt(cl) * 2
    b1 = torch.randn(S, generator=gn) * 0.5
    w2 = torch.randn((cl, S), generator=gn) / math.sqrt(S) * 3
    b2 = torch.randn(cl, generator=gn)
    ad, gd = a.cuda(), g.cuda()
    w1d, b1d, w2d, b2d = w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda()
    f = ops.se_train_forward(ad, w1d, b1d, w2d, b2d, gate_kind=gate_kind)
    d = lambda t: t.cpu().double()   # noqa: E731
    A64, G64, W1, B1, W2, B2 = a.double(), g.double(), w1.double(), b1.double(), w2.double(), b2.double()
    pooled, u1, h1, gate = d(f["pooled"]), d(f["u1"]), d(f["h1"]), d(f["gate"])
    _check_close(pooled, A64.mean(1), A64.abs().mean(1), "pooled", FP32)
    assert not bool(pooled[:, cl:].ne(0).any()) and not bool(gate[:, cl:].ne(0).any()), "pad columns"
    u1_ref = pooled[:, :cl] @ W1.t() + B1
    _check_close(u1, u1_ref, pooled[:, :cl].abs() @ W1.abs().t() + B1.abs(), "u1", FP32)
    if gate_kind:
        _assert_equal(f["h1"], u1.clamp(min=0), "h1 = relu(u1)")
    else:
        _check_close(h1, u1 / (1 + torch.exp(-u1)), u1.abs(), "h1", FP32)
    acc = h1 @ W2.t() + B2
    accA = h1.abs() @ W2.abs().t() + B2.abs()
    gate_ref = (acc + 3).clamp(0, 6) / 6 if gate_kind else 1 / (1 + torch.exp(-acc))
    _check_close(gate[:, :cl], gate_ref, accA, "gate", FP32)        # (both gates have slope <= 1/4)
    _check_close(f["out"], A64 * gate[:, None, :], (A64 * gate[:, None, :]).abs(), "out", BF16)
    # the gates from the squeeze that bna_apply_pool leaves: the same bits as pooling `a`
    chunks = ops.mbconv_geometry(2, c=C, hw=hw)[1]
    b = ops.se_train_backward(gd, ad, f, w1d, w2d, gate_kind=gate_kind)
    part = d(b["pool_part"])
    ga = (G64 * A64)
    rows = (hw + chunks - 1) // chunks
    for q in range(chunks):
        sl = slice(q * rows, min(hw, (q + 1) * rows))
        _check_close(part[:, q], ga[:, sl].sum(1), ga[:, sl].abs().sum(1), f"pool_part chunk {q}", FP32)
    dg = part.sum(1)
    if gate_kind:
        du2_ref = torch.where((gate > 0) & (gate < 1), dg / 6, torch.zeros_like(dg))
    else:
        du2_ref = dg * gate * (1 - gate)
    du2_ref[:, cl:] = 0
    du2 = d(b["du2"])
    _check_close(du2, du2_ref, part.abs().sum(1), "du2", FP32)
    t = du2[:, :cl] @ W2
    tA = du2[:, :cl].abs() @ W2.abs()
    if gate_kind:
        du1_ref = torch.where(u1 > 0, t, torch.zeros_like(t))
    else:
        s = 1 / (1 + torch.exp(-u1))
        du1_ref = t * s * (1 + u1 * (1 - s))
    du1 = d(b["du1"])
    _check_close(du1, du1_ref, tA * 1.1, "du1", FP32)
    dpool = du1 @ W1
    dpA = du1.abs() @ W1.abs()
    da_ref = G64 * gate[:, None, :]
    da_ref[:, :, :cl] += (dpool / hw)[:, None, :]
    Ada = (G64 * gate[:, None, :]).abs()
    Ada[:, :, :cl] += (dpA / hw)[:, None, :]
    _check_close(b["da"], da_ref, Ada, "da", BF16)
    _assert_pad_zero(b["da"], cl, "da")
    _check_close(b["gw2"], du2[:, :cl].t() @ h1, du2[:, :cl].abs().t() @ h1.abs(), "gW2", FP32)
    _check_close(b["gb2"], du2[:, :cl].sum(0), du2[:, :cl].abs().sum(0), "gb2", FP32)
    _check_close(b["gw1"], du1.t() @ pooled[:, :cl], du1.abs().t() @ pooled[:, :cl].abs(), "gW1", FP32)
    _check_close(b["gb1"], du1.sum(0), du1.abs().sum(0), "gb1", FP32)


@pytest.mark.parametrize("act", [ACT_SILU, ACT_RELU])
def test_squeeze_of_bna_apply_pool_feeds_the_gates(act):
    """bna_apply_pool's chunk sums are the sums of the rounded values it stores, in pool_rows' order: the gates
    computed from them are bit-identical to the gates computed by pooling its output."""
    from sykepic_hip import ops
    n, hw, C, cl, S = 5, 197, 320, 300, 20
    gn = _gen(101)
    raw = _zero_pad(torch.randn((n, hw, C), generator=gn).bfloat16(), cl)
    r = ops.bna_forward(raw.cuda(), (torch.rand(cl, generator=gn) + 0.5).cuda(), torch.randn(cl, generator=gn).cuda(),
                        torch.zeros(cl, device="cuda"), torch.ones(cl, device="cuda"), act=act, pool=True)
    out = r["out"]
    chunks = r["pool_part"].shape[1]
    rows = (hw + chunks - 1) // chunks
    o64 = out.cpu().double()
    part = r["pool_part"].cpu().double()
    for q in range(chunks):
        sl = slice(q * rows, min(hw, (q + 1) * rows))
        _check_close(part[:, q], o64[:, sl].sum(1), o64[:, sl].abs().sum(1), f"pool_part chunk {q}", FP32)
    w1, b1 = torch.randn((S, cl), generator=gn).cuda() * 0.1, torch.randn(S, generator=gn).cuda()
    w2, b2 = torch.randn((cl, S), generator=gn).cuda() * 0.3, torch.randn(cl, generator=gn).cuda()
    f1 = ops.se_train_forward(out, w1, b1, w2, b2, pool_part=r["pool_part"], want_out=False)
    f2 = ops.se_train_forward(out, w1, b1, w2, b2, want_out=False)
    for key in ("pooled", "u1", "h1", "gate"):
        assert torch.equal(f1[key], f2[key]), key


def test_exact_hardsigmoid_gate_on_its_kinks():
    """W2 = 0, b2 in {-3, 0, 3}: gate = 0, 1/2, 1 exactly; du2 = 0 where the gate sits on 0 or 1 (torch's
    hardsigmoid backward is 1/6 on the open interval only), dg / 6 in between."""
    from sykepic_hip import ops
    n, hw, C, cl, S = 2, 4, 64, 48, 8
    a = _zero_pad(_ints((n, hw, C), -3, 3, 111), cl)
    g = _zero_pad(_ints((n, hw, C), -3, 3, 112), cl)
    b2 = (torch.arange(cl) % 3 - 1).float() * 3
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    f = ops.se_train_forward(_dev(a), z(S, cl), z(S), z(cl, S), b2.cuda(), gate_kind=1)
    gate_ref = torch.zeros((n, C))
    gate_ref[:, :cl] = (b2 + 3) / 6
    _assert_equal(f["gate"], gate_ref, "gate")
    b = ops.se_train_backward(_dev(g), _dev(a), f, z(S, cl), z(cl, S), gate_kind=1)
    x = b2.clone().requires_grad_(True)
    dg = (a * g).sum(1, dtype=torch.int64).float()[:, :cl]
    F.hardsigmoid(x.expand(n, cl)).backward(dg)
    want = torch.zeros((n, C))
    want[:, :cl] = torch.where(b2 == 0, dg / 6, torch.zeros_like(dg))
    assert not bool(x.grad[b2 != 0].ne(0).any()) and bool(x.grad[b2 == 0].ne(0).any()), "torch's hardsigmoid' on +-3"
    got = b["du2"].cpu()
    assert torch.equal(got[:, :cl][:, b2 != 0], want[:, :cl][:, b2 != 0]), "du2 on the kinks"
    _check_close(got, want.double(), want.double().abs(), "du2", FP32)


@pytest.mark.parametrize("case", SE_WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_se_wgrad(case):
    from sykepic_hip import ops
    n, C, cl, S = case
    du2 = _zero_pad(_ints((n, C), -3, 3, 121), cl).long()
    pooled = _zero_pad(_ints((n, C), -3, 3, 122), cl).long()
    h1, du1 = _ints((n, S), -3, 3, 123).long(), _ints((n, S), -3, 3, 124).long()
    assert 9 * n < TWO24
    r = ops.se_wgrad(_dev(du2, torch.float32), _dev(h1, torch.float32), _dev(du1, torch.float32),
                     _dev(pooled, torch.float32), cl)
    _assert_equal(r["gw2"], du2[:, :cl].t() @ h1, "gW2")
    _assert_equal(r["gb2"], du2[:, :cl].sum(0), "gb2")
    _assert_equal(r["gw1"], du1.t() @ pooled[:, :cl], "gW1")
    _assert_equal(r["gb1"], du1.sum(0), "gb1")


def test_more_than_256_hidden_units_are_refused():
    from sykepic_hip import ops
    n, hw, C, cl, S = 1, 4, 64, 64, 257
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    a = torch.zeros((n, hw, C), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match=r"error -4"):
        ops.se_train_forward(a, z(S, cl), z(S), z(cl, S), z(cl))
    with pytest.raises(RuntimeError, match=r"error -4"):
        ops.se_wgrad(z(n, C), z(n, S), z(n, S), z(n, C), cl)
    with pytest.raises(RuntimeError, match=r"error -4"):
        ops.mbconv_geometry(3, m=cl, s=S)


# ---------------------------------------------------------------- stem
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_stem3_train(case):
    from sykepic_hip import ops
    n, h, w, cin, cout = case
    C = (cout + 63) // 64 * 64
    gn = _gen(131)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    px = torch.randint(0, 256, (n, h, w, cin), generator=gn)
    x4 = torch.zeros((n, h, w, 4), dtype=torch.bfloat16)
    x4[..., :cin] = px.bfloat16()
    assert torch.equal(x4[..., :cin].long(), px)
    wgt = torch.randn((cout, 9, cin), generator=gn) * 0.2
    dy = _zero_pad(torch.randn((n, ho, wo, C), generator=gn).bfloat16(), cout)
    r = ops.stem3_train(x4.cuda(), wgt.cuda(), C, dy=dy.cuda())
    xt = px.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = wgt.bfloat16().double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xt, wr, None, 2, 1) / 255
    yA = F.conv2d(xt.detach(), wr.detach().abs(), None, 2, 1) / 255
    y_ref = torch.zeros((n, ho, wo, C), dtype=torch.float64)
    A = torch.zeros_like(y_ref)
    y_ref[..., :cout], A[..., :cout] = y.detach().permute(0, 2, 3, 1), yA.permute(0, 2, 3, 1)
    _check_close(r["y"], y_ref, A, "y", BF16)
    _assert_pad_zero(r["y"], cout, "y")
    gd = dy[..., :cout].double().permute(0, 3, 1, 2)
    dw_ref = torch.autograd.grad(F.conv2d(xt, wr, None, 2, 1), wr, gd)[0] / 255
    dwA = torch.autograd.grad(F.conv2d(xt, wr, None, 2, 1), wr, gd.abs())[0] / 255
    got = r["dw"].cpu().double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    bound = 2.0 ** -14 * dwA
    worst = float(((got - dw_ref).abs() - bound).max())
    assert worst <= 0, f"dw: over its bound by {worst:.3e}"
