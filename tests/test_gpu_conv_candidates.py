"""Every implicit-GEMM candidate the tuner can pick, in every mode, against a float64 reference.

`spk_conv_launch` (csrc/conv_igemm.hip) times tile configs 0..6 x main-loop flavours 0/1/3/4/5/6 per problem, keeps
the fastest and hands it on to any batch within a factor of two, so a candidate also runs at pixel counts it was never
timed at.  The code's claim is that every candidate is correct for every M and that the choice only affects speed.
Here each problem runs under every (cfg, flavour) of the FULL grid (not the tuner's filtered list), pinned through
`ops.pinned_conv` (spk_op_conv_pin), and the weight gradient under both of its pipeline depths.

Per problem the reference is computed once, in float64 on the CPU, from the same rounded operands the kernel sees
(bf16 / fp16 activations; weights chosen so that the packed 16-bit image - hi + lo for the split fp16 weights - is
exact).  Three things are asserted:

1. Per element, for every candidate that ran: |got - ref| <= 2^-8 |ref| + 2^-16 A, where A is the float64
   convolution of |x| with |w| (one rounding of a 16-bit output plus fp32 accumulation, scaled per element).
   fp16 outputs use 2^-11 |ref| (fp16's unit roundoff) + 2^-16 A' + 2^-24 (subnormal spacing), A' also carrying the
   eval epilogue's |scale| A + |shift| + |shortcut|; float32 outputs (dw) 2^-20 |ref| + 2^-16 A.
2. Bit identity across candidates for every quantity the code claims is tile-independent: the raw conv output of the
   training forward, dx (all dgrad forms, the stored input gradient of the BN-fused dgrad included), dw, and the fp16
   eval output.  Tile-DEPENDENT quantities, through the grouping of the partial sums by M tile, are only bounded: the
   BatchNorm batch mean / invstd and running statistics of the forward (and through them its normalised output and
   ReLU mask), and dgamma / dbeta / the producer's dy of the BN-fused dgrad.  Their bounds: the statistics within
   2^-12 relative (of the rms for the mean) - fp32 sums of up to a few thousand terms; the normalised output within
   one bf16 rounding + 2^-10 of its terms' magnitudes (the statistics' error times the per-element scale); dgamma /
   dbeta within the per-element conv bound summed + 2^-14 of the sum of |terms|.
3. Coverage: every flavour instantiated for a mode ran in this file; a candidate returns "does not fit" exactly when
   its flavour is not instantiated for its (narrowed) tile - `instantiated` below mirrors the compile-time conditions
   of launch_hybrid / launch_bk32 - so no candidate the tuner can time for a problem is unsupported.

The padded-channel fp16 flavours of the EfficientNet path (`cin_s` / `cout_s`, with and without the squeeze-excitation
gates in the operand) run under the same candidate grid in tests/test_gpu_mbconv_eval_ops.py, which also holds the
operator tests of the dedicated stem kernel (conv_stem.hip; no tile choice) in its fp16 eval forms.
"""

import collections
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (BM, BN, WARPS_M, WARPS_N) of launch_with's configs
TILES = {0: (128, 128, 2, 2), 1: (256, 64, 4, 1), 2: (64, 64, 2, 2), 3: (128, 64, 2, 2), 4: (256, 128, 4, 2),
         5: (256, 256, 2, 4), 6: (256, 64, 4, 2)}
FLAVOURS = (0, 1, 3, 4, 5, 6)
GRID = [(c, f) for c in range(7) for f in FLAVOURS]
MODES = ("fwd_bn", "dgrad_s1", "dgrad_s2", "dgrad_bnb", "eval_1x1", "eval_3x3", "wgrad")

RAN = collections.defaultdict(set)        # mode -> {(narrowed tile config, flavour)}
PAIRS = collections.Counter()             # mode -> (problem, candidate) pairs that ran
UNSUPPORTED = collections.defaultdict(set)
T0 = [None]


def effective_cfg(cfg, cout, splitw):
    """launch_with's narrowing: 256x256 -> 256x128 (Cout % 256, split weights) -> 128x64 (Cout % 128)."""
    if cfg == 5 and (cout % 256 or splitw):
        cfg = 4
    if cfg in (0, 4) and cout % 128:
        cfg = 3
    return cfg


def instantiated(cfg, flav, cout, splitw):
    bm, bn, wm, wn = TILES[effective_cfg(cfg, cout, splitw)]
    nb = 2 if splitw else 1
    if flav == 4:   # launch_hybrid
        return bm * bn < 256 * 256 and not (bm == 256 and wn == 1) and (bm + nb * bn) * 128 * 2 <= 163840
    if flav == 5:   # launch_bk32
        g = wm * wn * 16
        return (wm * wn * 64 // 4) % 16 == 0 and bm % g == 0 and (nb * bn) % g == 0
    return True


def tuner_times(cfg, flav, m, cout, splitw):
    """The candidates spk_conv_launch's timing loop launches for a problem of m GEMM rows and cout GEMM columns."""
    bm, bn = TILES[cfg][:2]
    if cout % bn or (cfg == 5 and splitw) or (cfg == 1 and cout != 64) or (cfg == 6 and flav < 3):
        return False
    if bm > 64 and m < bm * 64 and ((m + bm - 1) // bm) * (cout // bn) < 128:
        return False
    return instantiated(cfg, flav, cout, splitw)


@pytest.fixture(scope="module", autouse=True)
def _unpinned():
    """No pin leaks into or out of this module, whatever a test does."""
    from sykepic_hip import lib
    so = lib.load()
    lib.check(so.spk_op_conv_pin(-1, -1, -1))
    T0[0] = time.perf_counter()
    yield
    lib.check(so.spk_op_conv_pin(-1, -1, -1))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).bfloat16()


def _f16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).half()


def _split_weights(shape, seed, split):
    """fp32 weights whose packed fp16 image is exact: w = h (+ l), h and l fp16, |l| < half an ulp of h and l normal,
    l's lowest bit no more than 23 below h's top bit (w exact in fp32), so pack's hi = fp16(w) = h and lo = fp16(w - hi)
    = l."""
    h = _f16(shape, seed).float()
    if not split:
        return h
    u = torch.rand(shape, generator=_gen(seed + 1)) * 2 - 1
    e = torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -24)))
    lo = torch.round(u * 2.0 ** 10) * torch.exp2(e - 22)
    lo = torch.where(lo.abs() >= 2.0 ** -14, lo, torch.zeros_like(lo))
    w = h + lo
    assert torch.equal(w.half().float(), h) and torch.equal((w - h).half().float(), lo)
    return w


def _mask_bits(pos):
    """[N,C,H,W] bool -> [M][C/8] uint8, bit j = channel 8*cc + j."""
    n, c, h, w = pos.shape
    p = pos.permute(0, 2, 3, 1).reshape(n * h * w, c // 8, 8).to(torch.uint8)
    weights = (2 ** torch.arange(8, dtype=torch.int32)).to(torch.uint8)
    return (p * weights).sum(-1).to(torch.uint8)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class Sweep:
    """Runs `run()` under every candidate of the grid and collects what the checks below need."""

    def __init__(self, mode, name, m, cout, splitw=False):
        self.mode, self.name, self.m, self.cout, self.splitw = mode, name, m, cout, splitw
        self.fail = []
        self.groups = {}   # quantity -> list of (representative tensor, [candidates])

    def run(self, run):
        from sykepic_hip import ops
        out = {}
        for cfg, fl in GRID:
            cand = (cfg, fl)
            try:
                with ops.pinned_conv(cfg, fl):
                    res = run()
                torch.cuda.synchronize()
            except RuntimeError as e:
                if "does not fit" not in str(e):
                    raise
                UNSUPPORTED[self.mode].add((effective_cfg(cfg, self.cout, self.splitw), fl))
                assert not tuner_times(cfg, fl, self.m, self.cout, self.splitw), \
                    f"{self.mode} {self.name}: the tuner times cfg {cfg} flavour {fl} but it returned unsupported"
                assert not instantiated(cfg, fl, self.cout, self.splitw), \
                    f"{self.mode} {self.name}: cfg {cfg} flavour {fl} is instantiated but returned unsupported: {e}"
                continue
            assert instantiated(cfg, fl, self.cout, self.splitw), \
                f"{self.mode} {self.name}: cfg {cfg} flavour {fl} ran although its flavour is not instantiated for the tile"
            RAN[self.mode].add((effective_cfg(cfg, self.cout, self.splitw), fl))
            PAIRS[self.mode] += 1
            out[cand] = res
        assert out, f"{self.mode} {self.name}: no candidate ran"
        return out

    def bound(self, cand, what, got, ref, bound):
        """Per-element |got - ref| <= bound (NaN / unwritten elements fail)."""
        err = (got.double() - ref).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            self.fail.append(f"cfg {cand[0]} flavour {cand[1]}: {what}: {int(bad.sum())} of {bad.numel()} elements out of "
                             f"bound (first: flat {i}, got {float(got.flatten()[i]):.6g}, ref {float(ref.flatten()[i]):.6g}, "
                             f"bound {float(bound.flatten()[i]):.3g})")

    def same_bits(self, cand, what, got):
        for rep, members in self.groups.setdefault(what, []):
            if torch.equal(_bits(rep), _bits(got)):
                members.append(cand)
                return
        self.groups[what].append((got, [cand]))

    def finish(self):
        for what, groups in self.groups.items():
            if len(groups) > 1:
                desc = "; ".join(f"{len(m)} candidate(s) {m[:6]}{'...' if len(m) > 6 else ''}"
                                 for _, m in sorted(groups, key=lambda g: -len(g[1])))
                self.fail.append(f"{what} is not bit-identical across candidates: {len(groups)} groups: {desc}")
        assert not self.fail, f"{self.mode} {self.name}:\n  " + "\n  ".join(self.fail[:20])


def _bf16_bound(ref, a):
    return ref.abs() * 2.0 ** -8 + a * 2.0 ** -16


def _gpu(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------------------------------
# bf16 forward + BatchNorm statistics (spk_op_conv_bn_train_forward)
# ------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, k, stride, pad, res, relu)
FWD = [
    (1, 7, 7, 64, 64, 1, 1, 0, False, True),          # M 49 < every tile, K 64
    (1, 15, 17, 64, 128, 3, 1, 1, True, True),        # M 255, K 576
    (1, 16, 16, 2048, 256, 1, 1, 0, False, False),    # M 256, K 2048, Cout 256
    (1, 1, 257, 512, 64, 3, 1, 1, True, False),       # M 257, K 4608
    (1, 16, 16, 64, 2048, 1, 1, 0, False, True),      # Cout 2048 (256x256 tile), K 64
    (2, 15, 13, 64, 128, 3, 2, 1, False, True),       # stride 2, M 112
    (8, 28, 28, 64, 64, 3, 1, 1, True, True),         # whole tiles: M 6272
]


@pytest.mark.parametrize("case", FWD, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_res%d_relu%d" % c)
def test_forward_bn_every_candidate(case):
    from sykepic_hip import ops
    n, h, w, cin, cout, k, stride, pad, with_res, relu = case
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    m = n * oh * ow
    x = _bf16((n, cin, h, w), 1)
    wt = _bf16((cout, cin, k, k), 2, (2.0 / (cin * k * k)) ** 0.5)
    res = _bf16((n, cout, oh, ow), 3) if with_res else None
    gamma = torch.randn(cout, generator=_gen(4)) * 0.5 + 1.0
    beta = torch.randn(cout, generator=_gen(5)) * 0.3
    rm0 = torch.randn(cout, generator=_gen(6)) * 0.1
    rv0 = torch.rand(cout, generator=_gen(7)) + 0.5

    x64, w64 = x.double(), wt.double()
    ref = F.conv2d(x64, w64, stride=stride, padding=pad)
    a = F.conv2d(x64.abs(), w64.abs(), stride=stride, padding=pad)
    mean = ref.mean((0, 2, 3))
    var = ref.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    rms = ref.pow(2).mean((0, 2, 3)).sqrt()
    rm_ref = 0.9 * rm0.double() + 0.1 * mean
    rv_ref = 0.9 * rv0.double() + 0.1 * var * m / (m - 1)
    ref_g, bound_g = _gpu(ref), _gpu(_bf16_bound(ref, a))
    xg, wg, gg, bg = _gpu(x), _gpu(wt), _gpu(gamma), _gpu(beta)
    resg = _gpu(res) if with_res else None
    mean_g, invstd_g = _gpu(mean), _gpu(invstd)
    sc_g = invstd_g * _gpu(gamma.double())

    sw = Sweep("fwd_bn", str(case), m, cout)

    def run():
        rm, rv = _gpu(rm0.clone()), _gpu(rv0.clone())
        o = ops.conv_bn_train_forward(xg, wg, gg, bg, rm, rv, res=resg, relu=relu, stride=stride, pad=pad)
        return o, rm, rv

    for cand, (o, rm, rv) in sw.run(run).items():
        raw = o["raw"]
        sw.bound(cand, "raw", raw, ref_g, bound_g)
        sw.same_bits(cand, "raw", raw)
        sw.bound(cand, "mean", o["mean"], mean_g, _gpu(rms * 2.0 ** -12 + a.mean((0, 2, 3)) * 2.0 ** -16))
        sw.bound(cand, "invstd", o["invstd"], invstd_g, invstd_g * 2.0 ** -12)
        sw.bound(cand, "running_mean", rm, _gpu(rm_ref), _gpu(0.1 * (rms * 2.0 ** -12 + a.mean((0, 2, 3)) * 2.0 ** -16)
                                                             + rm_ref.abs() * 2.0 ** -20))
        sw.bound(cand, "running_var", rv, _gpu(rv_ref), _gpu(rv_ref.abs() * 2.0 ** -12))
        # the normalised output from this candidate's raw (bit-identical, checked above) and the float64 statistics
        r64 = raw.double()
        pre = (r64 - mean_g.view(1, -1, 1, 1)) * sc_g.view(1, -1, 1, 1) + _gpu(beta.double()).view(1, -1, 1, 1)
        mag = ((r64.abs() + mean_g.abs().view(1, -1, 1, 1)) * sc_g.abs().view(1, -1, 1, 1)
               + _gpu(beta.double()).abs().view(1, -1, 1, 1))
        if with_res:
            pre = pre + resg.double()
            mag = mag + resg.double().abs()
        want = pre.clamp_min(0) if relu else pre
        sw.bound(cand, "out", o["out"], want, want.abs() * 2.0 ** -8 + mag * 2.0 ** -10)
        if relu:
            if not torch.equal(o["mask"].cpu(), _mask_bits((o["out"] > 0).cpu())):
                sw.fail.append(f"cfg {cand[0]} flavour {cand[1]}: ReLU mask disagrees with the stored output")
    sw.finish()


# ------------------------------------------------------------------------------------------------------------------
# data gradient (spk_op_conv_dgrad): stride 1, and stride 2 by output parity class
# ------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, k, stride, pad, accumulate); the GEMM is M = n*h*w (per class at stride 2), K = k*k*cout, N = cin
DGRAD_S1 = [
    (1, 7, 7, 64, 64, 1, 1, 0, False),         # M 49, K 64
    (1, 15, 17, 128, 64, 3, 1, 1, True),       # M 255, K 576
    (1, 16, 16, 256, 2048, 1, 1, 0, False),    # M 256, K 2048, N 256
    (1, 1, 257, 64, 512, 3, 1, 1, True),       # M 257, K 4608
    (1, 8, 8, 2048, 64, 1, 1, 0, True),        # N 2048 (256x256 tile)
    (4, 28, 28, 128, 64, 3, 1, 1, False),      # whole tiles: M 3136
]
DGRAD_S2 = [
    (2, 15, 13, 64, 128, 3, 2, 1, False),      # odd h, w
    (2, 16, 16, 128, 64, 3, 2, 1, True),       # even h, w
    (2, 15, 16, 64, 64, 3, 2, 0, True),        # pad 0
    (2, 14, 14, 64, 256, 1, 2, 0, False),      # 1x1/2: three classes without taps (zeros)
    (1, 15, 15, 256, 64, 1, 2, 0, True),       # 1x1/2, odd, accumulate: base unchanged there
    (2, 9, 10, 64, 64, 1, 2, 1, False),        # 1x1/2 pad 1
]


def _dgrad_case(case, mode):
    from sykepic_hip import ops
    n, h, w, cin, cout, k, stride, pad, acc = case
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    wt = _bf16((cout, cin, k, k), 11, (2.0 / (cin * k * k)) ** 0.5).float()
    dy = _bf16((n, cout, oh, ow), 12)
    base = _bf16((n, cin, h, w), 13) if acc else None
    ref = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(), stride, pad)
    a = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double().abs(), dy.double().abs(), stride, pad)
    # pixels no tap reaches (1x1 / 2: three parity classes): exactly 0, or the accumulated base unchanged
    reach = torch.nn.grad.conv2d_input((1, 1, h, w), torch.ones(1, 1, k, k, dtype=torch.float64),
                                       torch.ones(1, 1, oh, ow, dtype=torch.float64), stride, pad)[0, 0] > 0
    if acc:
        ref = ref + base.double()
    ref_g, bound_g, reach_g = _gpu(ref), _gpu(_bf16_bound(ref, a)), _gpu(reach)
    dyg, wg = _gpu(dy), _gpu(wt)
    baseg = _gpu(base) if acc else None
    if stride == 1:
        m = n * h * w
    else:
        m = n * ((h + 1) // 2) * ((w + 1) // 2)
    sw = Sweep(mode, str(case), m, cin)
    for cand, dx in sw.run(lambda: ops.conv_dgrad(dyg, wg, (h, w), stride, pad, accumulate_into=baseg)).items():
        sw.bound(cand, "dx", dx, ref_g, bound_g)
        sw.same_bits(cand, "dx", dx)
        if not bool(reach.all()):
            dead = dx.permute(0, 2, 3, 1)[:, ~reach_g]
            want = baseg.permute(0, 2, 3, 1)[:, ~reach_g] if acc else torch.zeros_like(dead)
            if not torch.equal(_bits(dead), _bits(want)):
                sw.fail.append(f"cfg {cand[0]} flavour {cand[1]}: pixels no tap reaches are not "
                               f"{'the unchanged base' if acc else 'exactly zero'}")
    sw.finish()


@pytest.mark.parametrize("case", DGRAD_S1, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_acc%d" % c)
def test_dgrad_stride1_every_candidate(case):
    _dgrad_case(case, "dgrad_s1")


@pytest.mark.parametrize("case", DGRAD_S2, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_acc%d" % c)
def test_dgrad_stride2_parity_classes_every_candidate(case):
    _dgrad_case(case, "dgrad_s2")


# ------------------------------------------------------------------------------------------------------------------
# data gradient + the producer's BatchNorm backward (spk_op_conv_dgrad_bn_backward, CONV_MODE_DGRAD_BNB)
# ------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, k, pad, relu, res)
DGRAD_BNB = [
    (1, 7, 7, 64, 64, 1, 0, True, False),        # M 49, K 64
    (1, 15, 17, 128, 64, 3, 1, True, True),      # M 255, K 576
    (1, 16, 16, 256, 2048, 1, 0, False, True),   # M 256, K 2048
    (1, 1, 257, 64, 512, 3, 1, False, False),    # M 257, K 4608
    (4, 28, 28, 128, 64, 3, 1, True, False),     # whole tiles
]


@pytest.mark.parametrize("case", DGRAD_BNB, ids=lambda c: "n%d_%dx%d_c%d-%d_k%dp%d_relu%d_res%d" % c)
def test_dgrad_bn_backward_every_candidate(case):
    from sykepic_hip import ops
    n, h, w, cin, cout, k, pad, relu, with_res = case
    m = n * h * w
    wt = _bf16((cout, cin, k, k), 21, (2.0 / (cin * k * k)) ** 0.5).float()
    dy = _bf16((n, cout, h, w), 22)
    raw = (_bf16((n, cin, h, w), 23).float() * 1.7 + 0.4).bfloat16()
    gamma = torch.randn(cin, generator=_gen(24)) * 0.5 + 1.0
    mean = raw.double().mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(raw.double().var((0, 2, 3), unbiased=False) + 1e-5)).float()
    pos = torch.rand((n, cin, h, w), generator=_gen(25)) < 0.6 if relu else torch.ones((n, cin, h, w), dtype=torch.bool)
    res_src = _bf16((n, cin, h, w), 26) if with_res else None
    res_pos = torch.rand((n, cin, h, w), generator=_gen(27)) < 0.5

    g = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(), 1, pad)
    a = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double().abs(), dy.double().abs(), 1, pad)
    if with_res:
        g = g + res_src.double() * res_pos
    p64 = pos.double()
    xhat = (raw.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
    dbeta = (g * p64).sum((0, 2, 3))
    dgamma = (g * p64 * xhat).sum((0, 2, 3))
    conv_err = a * 2.0 ** -16 * p64
    dbeta_bound = conv_err.sum((0, 2, 3)) + (g * p64).abs().sum((0, 2, 3)) * 2.0 ** -14
    dgamma_bound = (conv_err * xhat.abs()).sum((0, 2, 3)) + (g * p64 * xhat).abs().sum((0, 2, 3)) * 2.0 ** -14
    gi = (gamma.double() * invstd.double()).view(1, -1, 1, 1)

    g_ref, g_bound = _gpu(g), _gpu(_bf16_bound(g, a))
    dyg, wg, rawg = _gpu(dy), _gpu(wt), _gpu(raw)
    maskg = _gpu(_mask_bits(pos))
    meang, invg, gammag = _gpu(mean), _gpu(invstd), _gpu(gamma)
    rsg = _gpu(res_src) if with_res else None
    rbg = _gpu(_mask_bits(res_pos)) if with_res else None
    xhat_g, p_g, gi_g = _gpu(xhat), _gpu(p64), _gpu(gi)
    dbeta_g, dgamma_g = _gpu(dbeta), _gpu(dgamma)

    sw = Sweep("dgrad_bnb", str(case), m, cin)
    run = lambda: ops.conv_dgrad_bn_backward(dyg, wg, (h, w), rawg, maskg, meang, invg, gammag, pad=pad, relu=relu,  # noqa: E731
                                             res_src=rsg, res_bits=rbg)
    for cand, o in sw.run(run).items():
        sw.bound(cand, "g (stored input gradient)", o["g"], g_ref, g_bound)
        sw.same_bits(cand, "g (stored input gradient)", o["g"])
        sw.bound(cand, "dbeta", o["dbeta"], dbeta_g, _gpu(dbeta_bound))
        sw.bound(cand, "dgamma", o["dgamma"], dgamma_g, _gpu(dgamma_bound))
        # the producer's dy from this candidate's stored g (bit-identical, checked above) and the float64 sums
        dz = o["g"].double() * p_g
        want = gi_g * (dz - dbeta_g.view(1, -1, 1, 1) / m - xhat_g * dgamma_g.view(1, -1, 1, 1) / m)
        mag = gi_g.abs() * (dz.abs() + dbeta_g.abs().view(1, -1, 1, 1) / m + (xhat_g * dgamma_g.view(1, -1, 1, 1)).abs() / m)
        sw.bound(cand, "dy (producer)", o["dy"], want, want.abs() * 2.0 ** -8 + mag * 2.0 ** -12)
    sw.finish()


# ------------------------------------------------------------------------------------------------------------------
# fp16 eval convolutions on the implicit GEMM (spk_op_conv1x1 / spk_op_conv3x3 with cfg < 0)
# ------------------------------------------------------------------------------------------------------------------
def _eval_case(mode, case, k):
    from sykepic_hip import ops
    n, h, w, cin, cout, stride, split, with_res = case
    pad = 1 if k == 3 else 0
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x = _f16((n, cin, h, w), 31)
    wt = _split_weights((cout, cin, k, k), 32, split)
    scale = torch.rand(cout, generator=_gen(34)) + 0.5
    shift = torch.randn(cout, generator=_gen(35)) * 0.2
    res = _f16((n, cout, oh, ow), 36) if with_res else None
    conv = F.conv2d(x.double(), wt.double(), stride=stride, padding=pad)
    a = F.conv2d(x.double().abs(), wt.double().abs(), stride=stride, padding=pad)
    s64, b64 = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    pre = conv * s64 + b64
    mag = a * s64.abs() + b64.abs()
    if with_res:
        pre = pre + res.double()
        mag = mag + res.double().abs()
    ref = pre.clamp_min(0)
    bound = ref.abs() * 2.0 ** -11 + mag * 2.0 ** -16 + 2.0 ** -24
    ref_g, bound_g = _gpu(ref), _gpu(bound)
    xg, wg, sg, bg = _gpu(x), _gpu(wt), _gpu(scale), _gpu(shift)
    rg = _gpu(res) if with_res else None
    sw = Sweep(mode, str(case), n * oh * ow, cout, splitw=bool(split))
    if k == 1:
        run = lambda: ops.conv1x1(xg, wg, sg, bg, stride=stride, relu=True, res=rg, split=bool(split), cfg=-1)  # noqa: E731
    else:
        run = lambda: ops.conv3x3(xg, wg, sg, bg, relu=True, split=bool(split), cfg=-1, res=rg)  # noqa: E731
    for cand, y in sw.run(run).items():
        sw.bound(cand, "y", y, ref_g, bound_g)
        sw.same_bits(cand, "y", y)
    sw.finish()


# (n, h, w, cin, cout, stride, split, res)
EVAL_1X1 = [
    (1, 7, 7, 64, 64, 1, 0, True),          # M 49, K 64
    (1, 15, 17, 256, 128, 1, 1, False),     # M 255, split weights
    (2, 16, 16, 64, 2048, 2, 0, False),     # stride 2, Cout 2048, K 64
    (1, 16, 16, 2048, 256, 1, 1, True),     # M 256, K 2048, split (256x256 narrowed to 256x128)
    (1, 1, 257, 128, 256, 1, 0, True),      # M 257, Cout 256
    (4, 28, 28, 128, 256, 2, 0, True),      # stride 2, M 784
]
# (n, h, w, cin, cout, stride 1, split, res)
EVAL_3X3 = [
    (1, 15, 17, 64, 64, 1, 0, True),        # M 255, K 576
    (1, 1, 257, 512, 64, 1, 1, False),      # M 257, K 4608, split
    (1, 7, 7, 256, 256, 1, 1, True),        # M 49, Cout 256, split
    (1, 16, 16, 128, 256, 1, 0, False),     # M 256, Cout 256 (256x256 tile)
    (4, 28, 28, 64, 128, 1, 0, False),      # whole tiles
]


@pytest.mark.parametrize("case", EVAL_1X1, ids=lambda c: "n%d_%dx%d_c%d-%d_s%d_split%d_res%d" % c)
def test_eval_conv1x1_every_candidate(case):
    _eval_case("eval_1x1", case, 1)


@pytest.mark.parametrize("case", EVAL_3X3, ids=lambda c: "n%d_%dx%d_c%d-%d_s%d_split%d_res%d" % c)
def test_eval_conv3x3_every_candidate(case):
    _eval_case("eval_3x3", case, 3)


# ------------------------------------------------------------------------------------------------------------------
# weight gradient (spk_op_conv_wgrad), both pipeline depths
# ------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, k, stride, pad)
WGRAD = [
    (2, 32, 32, 3, 64, 7, 2, 3),            # the 7x7/2 stem
    (3, 37, 29, 3, 64, 7, 2, 3),            # the stem, odd sizes
    (1, 15, 17, 64, 128, 3, 1, 1),          # M 255
    (2, 14, 14, 64, 64, 1, 2, 0),           # 1x1/2, K 64
    (1, 16, 16, 256, 2048, 1, 1, 0),        # Cin 256, Cout 2048
    (2, 9, 11, 128, 64, 3, 1, 1),           # Cin 128
    (4, 28, 28, 64, 64, 3, 1, 1),           # M 3136
]


@pytest.mark.parametrize("case", WGRAD, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d" % c)
def test_wgrad_both_pipelines(case):
    from sykepic_hip import ops
    n, h, w, cin, cout, k, stride, pad = case
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x = _bf16((n, cin, h, w), 41)
    dy = _bf16((n, cout, oh, ow), 42)
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), stride, pad)
    a = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, cin, k, k), dy.double().abs(), stride, pad)
    ref_g, bound_g = _gpu(ref), _gpu(ref.abs() * 2.0 ** -20 + a * 2.0 ** -16)
    xg, dyg = _gpu(x), _gpu(dy)
    sw = Sweep("wgrad", str(case), n * oh * ow, cout)
    for nb in (1, 2):
        with ops.pinned_conv(-1, -1, nb):
            dw = ops.conv_wgrad(xg, dyg, k, stride, pad)
        torch.cuda.synchronize()
        RAN["wgrad"].add(("nbuf", nb))
        PAIRS["wgrad"] += 1
        sw.bound(("nbuf", nb), "dw", dw, ref_g, bound_g)
        sw.same_bits(("nbuf", nb), "dw", dw)
    sw.finish()


def test_pin_rejects_bad_arguments_and_lifts():
    """cfg and flavour go together; the context manager lifts the pin even when its block raises."""
    from sykepic_hip import lib, ops
    so = lib.load()
    for args in ((3, -1, -1), (-1, 3, -1), (7, 0, -1), (0, 7, -1), (0, -1, 1), (-1, -1, 3)):
        assert so.spk_op_conv_pin(*args) != 0, args
    x = _bf16((1, 64, 7, 7), 51).cuda()
    wt = _bf16((64, 64, 1, 1), 52).float().cuda()
    with pytest.raises(RuntimeError, match="does not fit"):
        with ops.pinned_conv(1, 4):     # the hybrid flavour has no 256x64 / 4x1-wave form
            ops.conv_dgrad(x, wt, (7, 7))
    ops.conv_dgrad(x, wt, (7, 7))       # unpinned again: the tuner's choice runs


def test_coverage():
    """Runs last: every flavour instantiated for a mode ran in this file, and both weight-gradient pipelines."""
    missing = [m for m in MODES if not RAN[m]]
    if missing:
        pytest.skip(f"the sweeps of {missing} did not run in this session (run the whole file)")
    total = sum(PAIRS.values())
    print(f"\n(problem, candidate) pairs that ran: {total} in {time.perf_counter() - T0[0]:.1f} s")
    for mode in MODES:
        tiles = sorted(RAN[mode])
        print(f"  {mode:10s} {PAIRS[mode]:5d} pairs, {len(tiles):3d} distinct (tile, flavour): {tiles}")
        if UNSUPPORTED[mode]:
            print(f"  {'':10s} not instantiated (unsupported as expected): {sorted(UNSUPPORTED[mode])}")
    for mode in MODES:
        if mode == "wgrad":
            assert RAN[mode] == {("nbuf", 1), ("nbuf", 2)}
            continue
        flavours = {f for _, f in RAN[mode]}
        assert flavours == set(FLAVOURS), f"{mode}: flavours {sorted(set(FLAVOURS) - flavours)} never ran"
        assert {c for c, _ in RAN[mode]} == set(TILES), f"{mode}: tiles {sorted(set(TILES) - {c for c, _ in RAN[mode]})} never ran"
