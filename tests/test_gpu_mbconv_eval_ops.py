"""The MBConv EVAL kernels and the eval stems one operator at a time, at the launch branches production takes.

The kernels that produce EfficientNet / MobileNetV3 / ResNet probabilities and that the suite only saw through whole
networks - the padded-channel fp16 implicit GEMM with and without the squeeze-excitation gates in its operand
(csrc/conv_igemm.hip, PADC / GATE) and `pack_padded_kernel`, `se_fc1_kernel` / `se_fc2_kernel` / `se_scale_kernel` and the
3x3/2 RGB stem (csrc/effnet.hip, `pack_stem3`), the 7x7/2 ResNet stem in fp16 with and without split weights and with
and without the fused max-pool (csrc/conv_stem.hip) - run here through the single-operator hooks
`spk_op_conv1x1_padded`, `spk_op_se_eval`, `spk_op_stem3_eval` and `spk_op_stem7_eval` (sykepic_hip/ops.py), which make
the pack and launch calls the model executor makes for ONE such layer through its own dispatch functions.  The wrappers
NaN-poison every output and give it a sentinel tail (at least one more pixel row) that must come back untouched.
Two kinds of test, with the meaning they have in tests/test_gpu_mbconv_train_ops.py.

1. EXACT (`test_exact_*`): integer-valued operands and an integer / float64-of-integers reference on the CPU.  Every
   partial sum is an integer (or a half integer) below 2^24 and every fp16 output has at most 11 significant bits, so
   the kernel must EQUAL the reference whatever the order of its sums: no tolerance.  Each test asserts both conditions
   on the reference first (sum of |terms| < 2^24; |value| <= 2048 for fp16 outputs, <= 1024 where gates of 1/2 make
   half integers).  Asserted exactly:
   - padded 1x1 conv: x in [-3, 3], w in [-2, 2], scale 1, integer bias, act none / ReLU, with and without an integer
     shortcut, with gates from {0, 1/2, 1, 2}, with and without split weights, under EVERY (tile config, flavour) of the
     full candidate grid (the `Sweep` loop of tests/test_gpu_conv_candidates.py); the candidates that ran are
     bit-identical; a candidate is refused exactly where `launch_with` / `launch_cfg` do not instantiate it
     (`expected_to_run`: padded path flavours 0, 3, 6; gated path flavour 0; else the rules of the unpadded GEMM);
   - squeeze-excitation with the ReLU / Hardsigmoid gates: hid = relu(W1 . mean + b1) from integer partials with hw a
     power of two; scale on weights built so that every integer pre-activation is <= -3, 0 or >= 3 (a third of the
     elements each, asserted on the reference): exactly 0, 1/2, 1; y = x * scale exactly; and on free integer weights
     scale == float32(clamp(t + 3, 0, 6)) * float32(1/6), the kernel's one rounding, for every element.  (The gate
     function cannot produce 2: `se_scale` sees {0, 1/2, 1}; the gate 2 is covered by the gated conv.)
   - 3x3 stem: pixels 0 ... 15, weights [-2, 2], BatchNorm scale 255 (the folded float32(255) * float32(1/255) is exactly
     1, asserted), act none / ReLU;  7x7 stem: pixels 0 ... 3, the un-fused output, and the POOL variant against
     max_pool2d(reference, 3, 2, 1) - its first check against a reference rather than against the un-fused kernel.
2. BOUNDED (`test_random_*`): normal operands against a float64 reference built from the same rounded operands
   (weights from `_split_weights`: the packed hi (+ lo) image is exact; the gated operand reproduced as
   (x.float() * gate).half(), the rounding the kernel claims to make).  With A' the float64 sum of the absolute terms of
   the pre-activation, |scale| conv(|x|, |w|) + |shift| + |shortcut|:
   - fp16 outputs: |got - ref| <= 2^-11 |ref| + L 2^-16 A' + 2^-24, L the activation's Lipschitz constant (none / ReLU
     1, SiLU 1.1, Hardswish 1.5), the bound the project already uses for fp16 eval outputs;
   - SiLU outputs carry EXP_TERM |ref| more for the device's fp32 exp and reciprocal (2^-20, the starting value; not
     re-measured);
   - Hardswish: elements whose float64 pre-activation lies within 2^-16 A' of +-3 are left out, at most 0.1 % (also
     counted without a GPU by tests/test_host_mbconv_eval_geometry.py); ReLU needs no exclusion (1-Lipschitz
     everywhere) and gets none;
   - hid, scale (fp32): 2^-20 |ref| + L 2^-16 sum |terms| (SiLU 1.1, sigmoid 1/4, hardsigmoid 1/6, ReLU 1), each stage
     from the operands the kernel itself left for it; y of `se_scale`: 2^-11 |ref| + 2^-24, one fp16 rounding of the
     float64 product with the device's own gates;
   - every output finite everywhere, every sentinel tail untouched (checked by the wrappers on every call), and - since
     the hidden vector sits directly behind n * c gates - a `se_fc2` write past n * c would land in `hid`, which is
     checked.
   The bounds are derived, none is taken from what the kernels give.

Coverage of the launch branches is asserted without a GPU by tests/test_host_mbconv_eval_geometry.py, which feeds the
case lists below through `spk_op_mbconv_eval_geometry` (the launchers' own helpers).

Not covered / not observable in any output:
- the image clamp `min(im, nim - 1)` of se_fc1 / se_fc2 and the `chan_ok` select of the padded main loop guard reads
  whose values are dropped (the surplus image is masked out; the weights behind cin_s are zero): removing either
  changes no output, only the addresses that are read.
- bf16 instantiations of these kernels (the eval path is fp16).

Wall time of this file on an MI355X: 4.1 s for its 184 tests (first run); the slowest are
test_exact_conv1x1_padded[16x96x1x7x7x0x0x0x0] (0.44 s: the first launch of the process),
test_random_conv1x1_padded[16x96x1x7x7x0x0x2x0] (0.27 s) and test_exact_se_scale_under_grid_cap (0.16 s, the one
12.6 M-element case), every other one under 0.1 s - a 42-candidate sweep of the padded conv takes about 20 ms.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_candidates import GRID, Sweep, _split_weights, effective_cfg, instantiated

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_SILU, ACT_HSWISH = 0, 1, 2, 3
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SILU: 1.1, ACT_HSWISH: 1.5}
EXP_TERM = 2.0 ** -20      # |ref| share allowed for the device's fp32 exp / rcp in SiLU (starting value, not re-measured)
TWO24 = 2 ** 24

# ---------------------------------------------------------------- cases (read by tests/test_host_mbconv_eval_geometry.py)
# padded 1x1 conv: stored (cin, cout); (40, 240) is there for the 256x256 tile on the padded path (GEMM couts 256)
PAD_PAIRS = [(16, 96), (96, 24), (24, 144), (144, 40), (240, 80), (672, 112), (1152, 320), (320, 1280), (8, 8), (40, 240)]
# project convs (gated); (96, 256): the 256x256 tile on the gated path
GATED_PAIRS = [(96, 24), (144, 40), (672, 112), (1152, 320), (96, 256)]
# (n, h, w): M 49 < every tile; 297 and 392 = no multiple of 64, a last tile past M, two images in one tile; 5 images of
# one pixel in one tile
PAD_SHAPES = [(1, 7, 7), (3, 9, 11), (2, 14, 14), (5, 1, 1)]


def _pad_cases(acts):
    """(cin, cout, n, h, w, res, split, act, gated)"""
    cases = []
    for i, (cin, cout) in enumerate(PAD_PAIRS):
        for split in (0, 1):
            cases.append((cin, cout) + PAD_SHAPES[(i + split) % 4] + ((i + split) % 2, split, acts[(i // 2 + split) % len(acts)], 0))
    for i, (cin, cout) in enumerate(GATED_PAIRS):
        for split in (0, 1):
            cases.append((cin, cout) + PAD_SHAPES[(i + 2 * split + 1) % 4] + ((i + split + 1) % 2, split,
                                                                            acts[(i + split) % len(acts)], 1))
    return cases


PAD_EXACT_CASES = _pad_cases((ACT_NONE, ACT_RELU))
PAD_RANDOM_CASES = _pad_cases((ACT_SILU, ACT_HSWISH, ACT_NONE, ACT_RELU))

# squeeze-excitation: (c, sq, gate kind) x n x pool-partial rows x hw -> (c, sq, kind, n, chunks, hw)
SE_LAYERS = [(32, 8, 0), (96, 4, 0), (144, 6, 0), (240, 10, 0), (672, 28, 0), (2688, 112, 0), (16, 8, 1), (72, 24, 1),
             (576, 144, 1), (960, 240, 1)]
SE_N = (1, 7, 8, 9, 19)
SE_CHUNKS = (1, 2, 3, 4, 5, 7, 8, 16)
SE_HW = (1, 49, 64)
SE_CASES = [(c, sq, kind, SE_N[(i + j) % 5], SE_CHUNKS[(i + 3 * j) % 8], SE_HW[(i + 2 * j) % 3])
            for j in (0, 1) for i, (c, sq, kind) in enumerate(SE_LAYERS)]
# exact: the same problems with the ReLU / Hardsigmoid gates and hw a power of two
SE_EXACT_CASES = [(c, sq, 1, n, chunks, 16 if hw == 49 else hw) for (c, sq, _, n, chunks, hw) in SE_CASES]
# se_scale under its grid cap: hw * c / 8 / 256 = 768 blocks per image > 4096 / n = 512 (the one case above 14 x 14;
# 128 x 128 and not 112 x 112 because the exact test wants hw a power of two)
SE_SCALE_CAP_CASE = (96, 4, 1, 8, 4, 128 * 128)

# 3x3 stem: (n, h, w, cout, act); cout 16, 24, 64: run-time divisions (GT 0), 32, 40, 48: GT 4, 5, 6
STEM3_COUTS = (16, 24, 32, 40, 48, 64)
STEM3_SIZES = [(9, 7), (32, 32), (33, 45), (2, 2)]
STEM3_EXACT_CASES = [(2, h, w, c, (ACT_NONE, ACT_RELU)[(i + j) % 2])
                     for i, c in enumerate(STEM3_COUTS) for j, (h, w) in enumerate(STEM3_SIZES) if (i + j) % 2 == 0 or j == 3]
STEM3_RANDOM_CASES = [(2, h, w, c, (ACT_SILU, ACT_HSWISH)[(i + j) % 2])
                      for i, c in enumerate(STEM3_COUTS) for j, (h, w) in enumerate(STEM3_SIZES) if (i + j) % 2 == 1 or j == 0]
# 7x7 stem: (n, h, w, split, pool)
STEM7_SIZES = [(1, 37, 53), (2, 64, 64), (3, 75, 101), (2, 30, 28)]
STEM7_CASES = [(n, h, w, split, pool) for (n, h, w) in STEM7_SIZES for split in (0, 1) for pool in (0, 1)]


def pad64(c):
    return (c + 63) // 64 * 64


def expected_to_run(cfg, fl, cin, cout, split, gated):
    """launch_with + launch_cfg (csrc/conv_igemm.hip) for a pinned candidate: the gated operand has the register-staged
    flavour only, the padded-channel path flavours 0, 3 and 6, a problem whose channels are multiples of 64 the
    unpadded GEMM's rules."""
    if gated:
        return fl == 0
    if cin % 64 or cout % 64:
        return fl in (0, 3, 6)
    return instantiated(cfg, fl, pad64(cout), split)


# ---------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).double()


def _choice(values, shape, seed):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=_gen(seed))]


def act64(pre, act):
    if act == ACT_RELU:
        return pre.clamp_min(0)
    if act == ACT_SILU:
        return pre * torch.sigmoid(pre)
    if act == ACT_HSWISH:
        return pre * (pre + 3).clamp(0, 6) / 6
    return pre


def fp16_bound(pre, mag, act):
    """(ref, bound, keep) of an fp16 eval output from its float64 pre-activation and the sum of its absolute terms."""
    ref = act64(pre, act)
    bound = ref.abs() * 2.0 ** -11 + LIPSCHITZ[act] * mag * 2.0 ** -16 + 2.0 ** -24
    keep = torch.ones_like(pre, dtype=torch.bool)
    if act == ACT_SILU:
        bound = bound + ref.abs() * EXP_TERM
    if act == ACT_HSWISH:
        keep = ((pre - 3).abs() > mag * 2.0 ** -16) & ((pre + 3).abs() > mag * 2.0 ** -16)
    return ref, bound, keep


def _seed(case):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(case)) % (2 ** 31)


def _cid(case):
    return "x".join(str(int(v)) for v in case)


# ------------------------------------------------------------------------------------------------------------------
# references (CPU only: the host test counts their kink exclusions)
# ------------------------------------------------------------------------------------------------------------------
def pad_conv_reference(case, exact):
    """Operands and the float64 pre-activation / sum of absolute terms of one padded-conv case."""
    cin, cout, n, h, w, with_res, split, act, gated = case
    s = _seed(case)
    if exact:
        x = _ints((n, cin, h, w), -3, 3, s).half()
        wt = _ints((cout, cin), -2, 2, s + 1).float()
        scale = torch.ones(cout)
        bias = _ints((cout,), -4, 4, s + 2).float()
        res = _ints((n, cout, h, w), -3, 3, s + 3).half() if with_res else None
        gate = _choice([0.0, 0.5, 1.0, 2.0], (n, cin), s + 4).float() if gated else None
    else:
        x = torch.randn((n, cin, h, w), generator=_gen(s)).half()
        wt = _split_weights((cout, cin), s + 1, split)
        scale = (torch.rand(cout, generator=_gen(s + 2)) + 0.5) / math.sqrt(cin)
        bias = torch.randn(cout, generator=_gen(s + 3)) * 0.5
        res = torch.randn((n, cout, h, w), generator=_gen(s + 4)).half() if with_res else None
        gate = torch.rand((n, cin), generator=_gen(s + 5)) * 1.5 if gated else None
    xe = (x.float() * gate[:, :, None, None]).half() if gated else x      # the operand the kernel claims to stage
    if exact and gated:
        assert torch.equal(xe.double(), x.double() * gate.double()[:, :, None, None])
    s64, b64 = scale.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    pre = torch.einsum("nchw,oc->nohw", xe.double(), wt.double()) * s64 + b64
    mag = torch.einsum("nchw,oc->nohw", xe.double().abs(), wt.double().abs()) * s64.abs() + b64.abs()
    if with_res:
        pre = pre + res.double()
        mag = mag + res.double().abs()
    return dict(x=x, w=wt, scale=scale, bias=bias, res=res, gate=gate, pre=pre, mag=mag)


def stem_images(n, h, w, top, seed):
    """Images on the k / 255 grid, k in 0 ... top; returns (x float32 [n,3,h,w], k float64)."""
    k = _ints((n, 3, h, w), 0, top, seed)
    return (k / 255.0).float(), k


def stem3_reference(case, exact):
    n, h, w, cout, act = case
    s = _seed(case)
    x, k = stem_images(n, h, w, 15 if exact else 255, s)
    if exact:
        wt = _ints((cout, 3, 3, 3), -2, 2, s + 1).float()
        scale = torch.full((cout,), 255.0)
        bias = _ints((cout,), -4, 4, s + 2).float()
    else:
        wt = torch.randn((cout, 3, 3, 3), generator=_gen(s + 1)) * (2.0 / 27) ** 0.5
        scale = torch.rand(cout, generator=_gen(s + 2)) * 4 + 2
        bias = torch.randn(cout, generator=_gen(s + 3)) * 0.5
    s64, b64 = (scale.double() / 255.0).view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    pre = F.conv2d(k, wt.double(), stride=2, padding=1) * s64 + b64
    mag = F.conv2d(k, wt.double().abs(), stride=2, padding=1) * s64.abs() + b64.abs()
    return dict(x=x, w=wt, scale=scale, bias=bias, pre=pre, mag=mag)


def stem7_reference(n, h, w, split, exact):
    s = _seed((n, h, w, split, int(exact)))
    x, k = stem_images(n, h, w, 3 if exact else 255, s)
    if exact:
        wt = _ints((64, 3, 7, 7), -2, 2, s + 1).float()
        scale = torch.full((64,), 255.0)
        bias = _ints((64,), -4, 4, s + 2).float()
    else:
        wt = _split_weights((64, 3, 7, 7), s + 1, split)
        scale = (torch.rand(64, generator=_gen(s + 3)) + 0.5) * 0.1
        bias = torch.randn(64, generator=_gen(s + 4)) * 0.2
    s64, b64 = (scale.double() / 255.0).view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    pre = F.conv2d(k, wt.double(), stride=2, padding=3) * s64 + b64
    mag = F.conv2d(k, wt.double().abs(), stride=2, padding=3) * s64.abs() + b64.abs()
    return dict(x=x, w=wt, scale=scale, bias=bias, pre=pre, mag=mag)


_STEM7_CACHE = {}


def _stem7_shared(n, h, w, split, exact):
    """One reference per (shape, split): shared by the un-fused and the POOL case, left unchanged."""
    key = (n, h, w, split, exact)
    if key not in _STEM7_CACHE:
        _STEM7_CACHE[key] = stem7_reference(n, h, w, split, exact)
    return _STEM7_CACHE[key]


def folded_stem_scale(scale):
    """float32(scale) * float32(1 / 255): what spk_commit (and the hooks) leave in the stem's epilogue scale."""
    return scale.float() * torch.tensor(1.0, dtype=torch.float32).div(torch.tensor(255.0, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------
# padded-channel 1x1 conv, with and without the gates, every candidate
# ------------------------------------------------------------------------------------------------------------------
RAN_PAD = set()       # (narrowed tile config, flavour, split, gated, padded) that ran


@pytest.fixture(scope="module", autouse=True)
def _unpinned():
    """No pin leaks into or out of this module, whatever a test does."""
    from sykepic_hip import lib
    so = lib.load()
    lib.check(so.spk_op_conv_pin(-1, -1, -1))
    yield
    lib.check(so.spk_op_conv_pin(-1, -1, -1))


class EvalSweep(Sweep):
    """`Sweep` of tests/test_gpu_conv_candidates.py with the refusal rule of the padded / gated path."""

    def __init__(self, case):
        cin, cout, n, h, w, _, split, _, gated = case
        super().__init__("eval_padded", _cid(case), n * h * w, pad64(cout), splitw=bool(split))
        self.cin, self.cout_s, self.gated = cin, cout, bool(gated)

    def run(self, run):
        from sykepic_hip import ops
        out = {}
        for cfg, fl in GRID:
            want = expected_to_run(cfg, fl, self.cin, self.cout_s, self.splitw, self.gated)
            try:
                with ops.pinned_conv(cfg, fl):
                    res = run()
                torch.cuda.synchronize()
            except RuntimeError as e:
                if "does not fit" not in str(e):
                    raise
                assert not want, f"{self.name}: cfg {cfg} flavour {fl} is instantiated but returned unsupported: {e}"
                continue
            assert want, f"{self.name}: cfg {cfg} flavour {fl} ran although the launcher does not instantiate it"
            RAN_PAD.add((effective_cfg(cfg, self.cout, self.splitw), fl, self.splitw, self.gated,
                         bool(self.cin % 64 or self.cout_s % 64)))
            out[(cfg, fl)] = res
        assert out, f"{self.name}: no candidate ran"
        return out


def _run_pad(case, o):
    from sykepic_hip import ops
    act, split = case[7], case[6]
    g = lambda t: t.cuda() if t is not None else None    # noqa: E731
    xg, wg, sg, bg, rg, gg = g(o["x"]), g(o["w"]), g(o["scale"]), g(o["bias"]), g(o["res"]), g(o["gate"])
    return lambda: ops.conv1x1_padded(xg, wg, sg, bg, act=act, res=rg, gate=gg, split=bool(split))


@pytest.mark.parametrize("case", PAD_EXACT_CASES, ids=_cid)
def test_exact_conv1x1_padded(case):
    act, gated = case[7], case[8]
    o = pad_conv_reference(case, exact=True)
    ref = act64(o["pre"], act)
    assert float(o["mag"].max()) < TWO24 and float(ref.abs().max()) <= (1024 if gated else 2048)
    assert torch.equal(ref.half().double(), ref)
    ref_g = ref.cuda()
    sw = EvalSweep(case)
    for cand, y in sw.run(_run_pad(case, o)).items():
        if not torch.equal(y.double(), ref_g):
            bad = y.double() != ref_g
            i = int(bad.flatten().nonzero()[0])
            sw.fail.append(f"cfg {cand[0]} flavour {cand[1]}: {int(bad.sum())} of {bad.numel()} elements differ (first: flat "
                           f"{i}, got {float(y.flatten()[i])}, ref {float(ref_g.flatten()[i])})")
        sw.same_bits(cand, "y", y)
    sw.finish()


@pytest.mark.parametrize("case", PAD_RANDOM_CASES, ids=_cid)
def test_random_conv1x1_padded(case):
    act = case[7]
    o = pad_conv_reference(case, exact=False)
    ref, bound, keep = fp16_bound(o["pre"], o["mag"], act)
    assert int((~keep).sum()) <= keep.numel() // 1000
    # elements left out are never out of bound
    ref_g, bound_g = ref.cuda(), torch.where(keep, bound, torch.full_like(bound, float("inf"))).cuda()
    sw = EvalSweep(case)
    for cand, y in sw.run(_run_pad(case, o)).items():
        assert bool(torch.isfinite(y).all()), f"cfg {cand[0]} flavour {cand[1]}: non-finite output"
        sw.bound(cand, "y", y, ref_g, bound_g)
        sw.same_bits(cand, "y", y)
    sw.finish()


def test_padded_conv_candidate_coverage():
    """Runs after the sweeps: every flavour the padded and the gated path instantiate ran, on every tile they narrow to."""
    if not RAN_PAD:
        pytest.skip("the sweeps did not run in this session (run the whole file)")
    for gated, flavours in ((False, {0, 3, 6}), (True, {0})):
        for split in (False, True):
            got = {(c, f) for (c, f, s, g, padded) in RAN_PAD if g == gated and s == split and (padded or gated)}
            tiles = {0, 1, 2, 3, 4, 6} | (set() if split else {5})
            assert got == {(c, f) for c in tiles for f in flavours}, (gated, split, sorted(got))


# ------------------------------------------------------------------------------------------------------------------
# squeeze-excitation
# ------------------------------------------------------------------------------------------------------------------
def _se_exact_operands(case, thirds):
    c, sq, kind, n, chunks, hw = case
    s = _seed(case) + (17 if thirds else 0)
    p = _ints((n, chunks, c), -1, 1, s)
    partial = p * hw                                    # sums over hw pixels whose mean is the integer p
    mean = p.sum(1)                                     # [n, c]
    w1 = _ints((sq, c), -2, 2, s + 1)
    b1 = _ints((sq,), -4, 4, s + 2)
    pre1 = mean @ w1.T + b1
    mag1 = mean.abs() @ w1.abs().T + b1.abs()
    hid = pre1.clamp_min(0)
    if thirds:
        # channel ch % 3: 0 -> a zero row (t = 0), 1 -> weights >= 0, bias 3 (t >= 3), 2 -> weights <= 0, bias -3 (t <= -3)
        cls = torch.arange(c) % 3
        w2 = _ints((c, sq), 0, 2, s + 3) * torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)[cls].view(-1, 1)
        b2 = torch.tensor([0.0, 3.0, -3.0], dtype=torch.float64)[cls]
    else:
        # even channels: dense weights; odd channels: one hidden unit, +-1 (t = b2 wherever that unit is off)
        w2 = _ints((c, sq), -2, 2, s + 3)
        hot = torch.zeros((c, sq), dtype=torch.float64)
        hot[torch.arange(c), torch.randint(0, sq, (c,), generator=_gen(s + 4))] = 1.0
        hot = hot * _choice([-1.0, 1.0], (c, 1), s + 5)
        w2[1::2] = hot[1::2]
        b2 = _ints((c,), -3, 3, s + 6)
    t = hid @ w2.T + b2
    mag2 = hid @ w2.abs().T + b2.abs()
    assert float(mag1.max()) < TWO24 and float(mag2.max()) < TWO24 and float(partial.abs().sum(1).max()) < TWO24
    return dict(partial=partial.float(), w1=w1.float(), b1=b1.float(), w2=w2.float(), b2=b2.float(), hid=hid, t=t)


def _hsig32(t):
    """The kernel's Hardsigmoid on an integer pre-activation: float32(clamp(t + 3, 0, 6)) * float32(1 / 6), one rounding."""
    return ((t + 3).clamp(0, 6).float() * torch.tensor(1.0, dtype=torch.float32).div(torch.tensor(6.0, dtype=torch.float32)))


def _exact_se(case, thirds, with_x):
    from sykepic_hip import ops
    c, sq, kind, n, chunks, hw = case
    o = _se_exact_operands(case, thirds)
    scale_ref = _hsig32(o["t"])
    if thirds:
        cls = [int((o["t"] <= -3).sum()), int((o["t"] == 0).sum()), int((o["t"] >= 3).sum())]
        assert sum(cls) == n * c and min(cls) >= (n * c) // 3 - n, cls       # a third each (c % 3 channels over, per image)
        want = torch.where(o["t"] <= -3, 0.0, torch.where(o["t"] == 0, 0.5, 1.0)).float()
        assert torch.equal(scale_ref, want)                                   # the one rounding lands on 0, 1/2, 1
        real_zero = scale_ref == 0
    x = None
    if with_x:
        x = _ints((n, hw, c), -64, 64, _seed(case) + 9).half()
    g = lambda v: v.cuda()    # noqa: E731
    r = ops.se_eval(g(o["partial"]), g(o["w1"]), g(o["b1"]), g(o["w2"]), g(o["b2"]), hw, gate_kind=1,
                    x=g(x) if with_x else None)
    hid, scale = r["hid"].cpu(), r["scale"].cpu()
    assert torch.equal(hid.double(), o["hid"]), f"hid: {int((hid.double() != o['hid']).sum())} of {hid.numel()} differ"
    assert torch.equal(scale, scale_ref), f"scale: {int((scale != scale_ref).sum())} of {scale.numel()} differ"
    if thirds:
        assert torch.equal(scale == 0, real_zero)                             # 0 on no real channel by accident
    if with_x:
        y_ref = x.double() * scale_ref.double().view(n, 1, c)
        assert torch.equal(y_ref.half().double(), y_ref)
        y = r["y"].cpu()
        assert torch.equal(y.double(), y_ref), f"y: {int((y.double() != y_ref).sum())} of {y.numel()} differ"


@pytest.mark.parametrize("case", SE_EXACT_CASES, ids=_cid)
def test_exact_se_gates_on_thirds(case):
    """hid, scale in {0, 1/2, 1} on weights that put a third of the pre-activations on each, y = x * scale."""
    _exact_se(case, thirds=True, with_x=True)


@pytest.mark.parametrize("case", SE_EXACT_CASES, ids=_cid)
def test_exact_se_gates_free_weights(case):
    """hid and every scale on free integer weights (the gates only: y == NULL)."""
    _exact_se(case, thirds=False, with_x=False)


def test_exact_se_scale_under_grid_cap():
    _exact_se(SE_SCALE_CAP_CASE, thirds=True, with_x=True)


@pytest.mark.parametrize("case", SE_CASES, ids=_cid)
def test_random_se(case):
    from sykepic_hip import ops
    c, sq, kind, n, chunks, hw = case
    s = _seed(case)
    partial = torch.randn((n, chunks, c), generator=_gen(s)) * math.sqrt(hw / chunks) + 0.3 * hw / chunks
    w1 = torch.randn((sq, c), generator=_gen(s + 1)) / math.sqrt(c)
    b1 = torch.randn((sq,), generator=_gen(s + 2)) * 0.5
    w2 = torch.randn((c, sq), generator=_gen(s + 3)) * 2 / math.sqrt(sq)
    b2 = torch.randn((c,), generator=_gen(s + 4))
    x = torch.randn((n, hw, c), generator=_gen(s + 5)).half()
    g = lambda v: v.cuda()    # noqa: E731
    r = ops.se_eval(g(partial), g(w1), g(b1), g(w2), g(b2), hw, gate_kind=kind, x=g(x))
    hid, scale, y = r["hid"].cpu(), r["scale"].cpu(), r["y"].cpu()
    for name, v in (("hid", hid), ("scale", scale), ("y", y)):
        assert bool(torch.isfinite(v).all()), f"{name}: non-finite"
    mean = partial.double().sum(1) / hw
    amean = partial.double().abs().sum(1) / hw
    pre1 = mean @ w1.double().T + b1.double()
    mag1 = amean @ w1.double().abs().T + b1.double().abs()
    hid_ref = pre1.clamp_min(0) if kind else pre1 * torch.sigmoid(pre1)
    l1 = 1.0 if kind else 1.1
    err = (hid.double() - hid_ref).abs()
    bound = hid_ref.abs() * 2.0 ** -20 + l1 * mag1 * 2.0 ** -16
    assert bool((err <= bound).all()), f"hid: {int((err > bound).sum())} out of bound, worst {float((err / bound).max()):.3g} x"
    # stage 2 from the hidden vector the kernel left
    pre2 = hid.double() @ w2.double().T + b2.double()
    mag2 = hid.double().abs() @ w2.double().abs().T + b2.double().abs()
    scale_ref = (pre2 + 3).clamp(0, 6) / 6 if kind else torch.sigmoid(pre2)
    l2 = 1.0 / 6 if kind else 0.25
    err = (scale.double() - scale_ref).abs()
    bound = scale_ref.abs() * 2.0 ** -20 + l2 * mag2 * 2.0 ** -16
    assert bool((err <= bound).all()), f"scale: {int((err > bound).sum())} out of bound, worst {float((err / bound).max()):.3g} x"
    # se_scale from the gates the kernel left: one fp16 rounding of the product
    y_ref = x.double() * scale.double().view(n, 1, c)
    err = (y.double() - y_ref).abs()
    bound = y_ref.abs() * 2.0 ** -11 + 2.0 ** -24
    assert bool((err <= bound).all()), f"y: {int((err > bound).sum())} out of bound, worst {float((err / bound).max()):.3g} x"


# ------------------------------------------------------------------------------------------------------------------
# the stems
# ------------------------------------------------------------------------------------------------------------------
def _assert_exact_fold():
    one = folded_stem_scale(torch.tensor([255.0]))
    assert float(one[0]) == 1.0, "float32(255) * float32(1 / 255) is not 1: the exact stem tests need another scale"


def _check_bounded(what, y, ref, bound, keep):
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
    assert int((~keep).sum()) <= keep.numel() // 1000, f"{what}: {int((~keep).sum())} elements near a kink"
    err = (y.double().cpu() - ref).abs()
    bad = keep & ~(err <= bound)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, worst "
                                 f"{float((err / bound)[keep].max()):.3g} x the bound")


@pytest.mark.parametrize("case", STEM3_EXACT_CASES, ids=_cid)
def test_exact_stem3(case):
    from sykepic_hip import ops
    _assert_exact_fold()
    act = case[4]
    o = stem3_reference(case, exact=True)
    ref = act64(o["pre"], act)
    assert float(o["mag"].max()) < TWO24 and float(ref.abs().max()) <= 2048 and torch.equal(ref, ref.round())
    y = ops.stem3_eval(o["x"].cuda(), o["w"].cuda(), o["scale"].cuda(), o["bias"].cuda(), act=act).cpu()
    assert torch.equal(y.double(), ref), f"{int((y.double() != ref).sum())} of {ref.numel()} elements differ"


@pytest.mark.parametrize("case", STEM3_RANDOM_CASES, ids=_cid)
def test_random_stem3(case):
    from sykepic_hip import ops
    act = case[4]
    o = stem3_reference(case, exact=False)
    ref, bound, keep = fp16_bound(o["pre"], o["mag"], act)
    y = ops.stem3_eval(o["x"].cuda(), o["w"].cuda(), o["scale"].cuda(), o["bias"].cuda(), act=act)
    _check_bounded("stem3", y, ref, bound, keep)


@pytest.mark.parametrize("case", STEM7_CASES, ids=_cid)
def test_exact_stem7(case):
    from sykepic_hip import ops
    _assert_exact_fold()
    n, h, w, split, pool = case
    o = _stem7_shared(n, h, w, split, True)
    ref = o["pre"].clamp_min(0)
    assert float(o["mag"].max()) < TWO24 and float(ref.abs().max()) <= 2048 and torch.equal(ref, ref.round())
    if pool:
        ref = F.max_pool2d(ref, 3, 2, 1)
    y = ops.stem7_eval(o["x"].cuda(), o["w"].cuda(), o["scale"].cuda(), o["bias"].cuda(), split=bool(split),
                       pool=bool(pool)).cpu()
    assert y.shape == ref.shape
    assert torch.equal(y.double(), ref), f"{int((y.double() != ref).sum())} of {ref.numel()} elements differ"


@pytest.mark.parametrize("case", STEM7_CASES, ids=_cid)
def test_random_stem7(case):
    from sykepic_hip import ops
    n, h, w, split, pool = case
    o = _stem7_shared(n, h, w, split, False)
    ref, bound, keep = fp16_bound(o["pre"], o["mag"], ACT_RELU)
    if pool:    # |max a - max b| <= max |a - b| over the window
        ref, bound = F.max_pool2d(ref, 3, 2, 1), F.max_pool2d(bound, 3, 2, 1)
        keep = torch.ones_like(ref, dtype=torch.bool)
    y = ops.stem7_eval(o["x"].cuda(), o["w"].cuda(), o["scale"].cuda(), o["bias"].cuda(), split=bool(split),
                       pool=bool(pool))
    assert y.shape == ref.shape
    _check_bounded("stem7", y, ref, bound, keep)
