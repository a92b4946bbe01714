"""`mix_kernel` (csrc/augment.hip) through `spk_mix_batch`: a batch mixed with a shifted copy of itself, against torch
on the CPU, BIT FOR BIT.

Oracle: inside the box `ca_t * a + cb_t * b` with 0-dim float32 tensors ca_t, cb_t - torch runs the two products and
the sum as three float32 ops, the roundings the kernel's `__fmul_rn` / `__fadd_rn` make - and for uint8 `torch.round`
(ties to even) of it, clamped to 0..255; outside the box the batch's own element; (ca, cb) = (0, 1) is the partner's
element itself, whatever its bits (-0.0 and denormals included).  b = a.roll(shift, 0).

Shapes: n of {1, 2, 5} x (h, w) of {(1, 1), (7, 9), (8, 8), (33, 20)} x c of {1, 3} x both layouts x shift of
{0, 1, n - 1}: images of 1 to 1980 elements, so chunks of 16 bytes that hold several images, straddle two, or lie
inside one; 7 * 9 * 3 = 189 bytes per image starts every second image at an odd address.  The input and the output
start 0 to 13 elements behind a 16-byte boundary (a partial first chunk), the output between guard bands.  uint8
images alternate in parity, so (0.5, 0.5) meets exact .5 ties whenever the partner is an odd number of images away.
"""

import pytest
import torch

import test_gpu_head_pool_ops as H

pytestmark = pytest.mark.gpu

NS = [1, 2, 5]
HWS = [(1, 1), (7, 9), (8, 8), (33, 20)]
CASES = [(n, h, w, c, u8) for n in NS for (h, w) in HWS for c in (1, 3) for u8 in (True, False)]
IDS = [f"{n}x{h}x{w}x{c}-{'u8nhwc' if u8 else 'f32nchw'}" for n, h, w, c, u8 in CASES]
GUARD_U8 = 0xA5


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


COEFFS = [(0.0, 1.0), (1.0, 0.0), (_f32(0.3), _f32(0.7)), (0.5, 0.5)]


def _boxes(h, w):
    ya, yb, xa, xb = h // 3, max(h // 3 + 1, 2 * h // 3), w // 3, max(w // 3 + 1, 2 * w // 3)
    boxes = [(0, 0, h, w), (0, 0, 0, 0), (h // 2, w // 2, h // 2, w // 2),                  # full, empty, empty inside
             (0, 0, 1, 1), (0, w - 1, 1, w), (h - 1, 0, h, 1), (h - 1, w - 1, h, w),        # one pixel at each corner
             (0, xa, yb, xb), (ya, xa, h, xb), (ya, 0, yb, xb), (ya, xa, yb, w),            # touching each edge
             (ya, xa, yb, xb)]                                                              # interior
    return list(dict.fromkeys(boxes))


def _batch(n, h, w, c, u8, seed):
    g = H._gen(seed)
    if u8:
        x = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.int64)
        parity = (torch.arange(n) % 2).view(n, 1, 1, 1)
        return ((x & ~1) | parity).clamp(0, 255).to(torch.uint8)        # image i holds numbers of parity i % 2
    return (torch.randn((n, c, h, w), generator=g, dtype=torch.float32) * 3).contiguous()


def _oracle(x, shift, ca, cb, box):
    a, b = x, x.roll(shift, 0)
    if (ca, cb) == (0.0, 1.0):
        m = b
    else:
        ca_t, cb_t = torch.tensor(ca, dtype=torch.float32), torch.tensor(cb, dtype=torch.float32)
        if x.dtype == torch.uint8:
            m = torch.round(ca_t * a.float() + cb_t * b.float()).clamp(0, 255).to(torch.uint8)
        else:
            m = ca_t * a + cb_t * b
    y1, x1, y2, x2 = box
    out = a.clone()
    if x.dtype == torch.uint8:
        out[:, y1:y2, x1:x2, :] = m[:, y1:y2, x1:x2, :]
    else:
        out[:, :, y1:y2, x1:x2] = m[:, :, y1:y2, x1:x2]
    return out


def _bits(t):
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _placed(x, lead):
    """x on the device, its first element `lead` elements behind a 256-byte boundary."""
    flat = torch.zeros(lead + x.numel(), dtype=x.dtype, device="cuda")
    view = flat[lead:].view(x.shape)
    view.copy_(x)
    return view


def _out_buffer(x, lead):
    """(flat, view): a device buffer of 64 guard elements, `lead` more, the output, and 64 + guard elements behind."""
    if x.dtype == torch.uint8:
        flat = torch.full((64 + lead + x.numel() + 80,), GUARD_U8, dtype=torch.uint8, device="cuda")
    else:
        flat = torch.full((64 + lead + x.numel() + 80,), H.SENTINEL, dtype=torch.float32, device="cuda")
    return flat, flat[64 + lead:64 + lead + x.numel()].view(x.shape)


def _guards_intact(flat, x, lead):
    f = flat.cpu()
    guard = GUARD_U8 if x.dtype == torch.uint8 else H.SENTINEL
    return bool((f[:64 + lead] == guard).all()) and bool((f[64 + lead + x.numel():] == guard).all())


@pytest.mark.parametrize("n,h,w,c,u8", CASES, ids=IDS)
def test_bit_exact_against_torch(n, h, w, c, u8):
    from sykepic_hip import ops
    x = _batch(n, h, w, c, u8, 100 * n + 10 * h + c)
    in_lead = (3, 0, 5)[(n + h) % 3] if u8 else (1, 0, 3)[(n + h) % 3]
    xd = _placed(x, in_lead)
    ties = calls = 0
    for shift in sorted({0, 1 % n, n - 1}):
        for bi, box in enumerate(_boxes(h, w)):
            for ci, (ca, cb) in enumerate(COEFFS):
                lead = ((0, 1, 7, 13) if u8 else (0, 1, 2, 3))[(bi + ci + shift) % 4]
                flat, out = _out_buffer(x, lead)
                got = ops.mix_batch(xd, ca, cb, box, shift=shift, out=out)
                assert got is out
                want = _oracle(x, shift, ca, cb, box)
                what = f"shift {shift} box {box} coefficients ({ca}, {cb}) output lead {lead}"
                assert torch.equal(_bits(out.cpu()), _bits(want)), what
                assert _guards_intact(flat, x, lead), f"{what}: memory around the output was written"
                calls += 1
                if u8 and (ca, cb) == (0.5, 0.5) and box == (0, 0, h, w) and shift % 2 == 1:
                    mean = 0.5 * x.float() + 0.5 * x.roll(shift, 0).float()
                    ties += int((mean.frac() == 0.5).sum())
    assert torch.equal(_bits(xd.cpu()), _bits(x)), "the input batch was written"
    assert calls >= 2 * len(COEFFS)         # (a 1 x 1 image has two distinct boxes: full and empty)
    if u8 and n > 1:
        assert ties > 0, "no exact .5 tie among the uint8 means: the rounding rule was not exercised"
    # two identical calls: identical bits
    box, (ca, cb) = _boxes(h, w)[-1], COEFFS[2]
    a = ops.mix_batch(xd, ca, cb, box, shift=1 % n)
    b = ops.mix_batch(xd, ca, cb, box, shift=1 % n)
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape", [(2, 1, 7, 9), (5, 3, 33, 20), (2, 3, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_cutmix_copies_every_float32_bit_pattern(shape):
    """(0, 1) takes the copy branch: -0.0, denormals, infinities and NaN payloads of the partner arrive bit for bit, and
    what lies outside the box keeps the bits of the batch's own image."""
    from sykepic_hip import ops
    n, c, h, w = shape
    x = _batch(n, h, w, c, False, 5)
    special = torch.tensor([-0.0, 1e-40, -1e-42, 1.4e-45, float("inf"), float("-inf"), 3.4e38], dtype=torch.float32)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=H._gen(9))[:4 * special.numel()]
    flat[idx] = special.repeat(4)
    bits = x.view(torch.int32).clone()
    bits.view(-1)[int(idx[0])] = 0x7FC12345                    # a NaN with a payload
    x = bits.view(torch.float32)
    xd = x.cuda()
    for box in _boxes(h, w):
        out = ops.mix_batch(xd, 0.0, 1.0, box, shift=1)
        assert torch.equal(_bits(out.cpu()), _bits(_oracle(x, 1, 0.0, 1.0, box))), box


def test_image_sized_batch_many_blocks():
    """4 x 180 x 180 x 3 bytes (the loader's batch layout, 95 blocks of 256 chunks) and its float32 NCHW counterpart."""
    from sykepic_hip import ops
    for u8 in (True, False):
        x = _batch(4, 180, 180, 3, u8, 77)
        xd = x.cuda()
        for (ca, cb), box in (((0.0, 1.0), (31, 0, 160, 97)), ((_f32(0.3), _f32(0.7)), (0, 0, 180, 180)),
                              ((0.5, 0.5), (100, 50, 180, 180))):
            out = ops.mix_batch(xd, ca, cb, box, shift=1)
            assert torch.equal(_bits(out.cpu()), _bits(_oracle(x, 1, ca, cb, box))), (u8, ca, cb, box)


def test_refused_calls_on_device_tensors():
    from sykepic_hip import ops
    x = _batch(2, 8, 8, 3, True, 1).cuda()
    with pytest.raises(RuntimeError, match="overlap"):
        ops.mix_batch(x, 0.5, 0.5, (0, 0, 8, 8), out=x)
    with pytest.raises(RuntimeError, match="shift"):
        ops.mix_batch(x, 0.5, 0.5, (0, 0, 8, 8), shift=2)
    with pytest.raises(RuntimeError, match="box"):
        ops.mix_batch(x, 0.5, 0.5, (0, 0, 9, 8))
    with pytest.raises(RuntimeError, match="finite"):
        ops.mix_batch(x, float("nan"), 0.5, (0, 0, 8, 8))


@pytest.mark.parametrize("u8", [True, False], ids=["u8nhwc", "f32nchw"])
def test_batch_mix_call_is_the_kernel_on_its_own_plan(u8):
    from sykepic_hip import ops
    from sykepic_hip.mix import BatchMix, f32
    n, h, w = 5, 33, 20
    x = _batch(n, h, w, 3, u8, 21).cuda()
    y = H._ints((n,), 0, 9, 22).cuda()
    bm, twin = BatchMix(0.4, 1.0, prob=0.8, seed=3), BatchMix(0.4, 1.0, prob=0.8, seed=3)
    kinds = set()
    for _ in range(24):
        xm, ya, yb, lam = bm(x, y)
        p = twin.plan(n, h, w)
        kinds.add(None if p is None else p.kind)
        assert torch.equal(ya, y)
        if p is None:
            assert xm is x and yb is None and lam == 1.0
            continue
        assert torch.equal(_bits(xm), _bits(ops.mix_batch(x, p.ca, p.cb, p.box, shift=1)))
        assert torch.equal(yb, y.roll(1)) and lam == f32(p.lam) and 0.0 <= lam <= 1.0
        assert xm.data_ptr() != x.data_ptr()
    assert kinds == {None, "mixup", "cutmix"}
    # a batch of one mixes with itself
    one = BatchMix(0.0, 1.0, seed=1)
    xm, ya, yb, lam = one(x[:1].contiguous(), y[:1])
    assert torch.equal(_bits(xm), _bits(x[:1])) and torch.equal(yb, y[:1])
