"""`tta_views_kernel` and `tta_mean_kernel` (csrc/tta.hip) through `spk_tta_views` / `spk_tta_mean`, against torch on
the CPU, BIT FOR BIT (float tensors are compared as int32).

Views.  Oracle: `transpose(H, W)` when the code has bit value 4, then `flip(H)` for bit value 2, then `flip(W)` for bit
value 1.  Shapes: n of {1, 2, 5} x (h, w) of {(1, 1), (7, 9), (8, 8), (33, 20), (33, 33), (65, 65)} x c of {1, 3} x
both batch kinds: images smaller than, straddling and beyond one LDS tile (32 pixels for float32, 64 for three-byte
pixels; the 128-pixel tile of one-byte pixels is straddled by the further shapes of `BIG`, with the same leads and
guard bands, and by the 180 x 180 case), odd row lengths in bytes, images that start at odd addresses.  View lists: each single code, `flip`, `dihedral` where the image is square, a list with
a duplicate.  The input and the output start 0 to 13 elements behind a 16-byte boundary; the output lies between guard
bands, which must stay intact; the input must be unwritten afterwards.

Mean.  Oracle: the explicit float32 loop `s = p[0]; s = s + p[j] ...` on the CPU, then `/ k` (torch's float32 add and
division are the IEEE operations).  k of {1, 2, 3, 4, 8} x numel of {1, 50, 150, 1027}.  For k >= 3 the reversed-order
sum must differ from the oracle somewhere - a property of the test's inputs, checked on the CPU - so a kernel that
sums in another order cannot pass.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 5]
HWS = [(1, 1), (7, 9), (8, 8), (33, 20), (33, 33), (65, 65)]
CASES = [(n, h, w, c, u8) for n in NS for (h, w) in HWS for c in (1, 3) for u8 in (True, False)]
IDS = [f"{n}x{h}x{w}x{c}-{'u8nhwc' if u8 else 'f32nchw'}" for n, h, w, c, u8 in CASES]
GUARD_U8 = 0xA5
GUARD_F32 = -12345.0
FLIP, DIHEDRAL = (0, 1, 2, 3), (0, 1, 2, 3, 4, 5, 6, 7)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _batch(n, h, w, c, u8, seed):
    g = _gen(seed)
    if u8:
        return torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.int64).to(torch.uint8)
    return (torch.randn((n, c, h, w), generator=g, dtype=torch.float32) * 3).contiguous()


def _view(x, v):
    """T_v of a uint8 [N,H,W,C] or float32 [N,C,H,W] CPU batch."""
    hd, wd = (1, 2) if x.dtype == torch.uint8 else (2, 3)
    if v & 4:
        x = x.transpose(hd, wd)
    if v & 2:
        x = x.flip(hd)
    if v & 1:
        x = x.flip(wd)
    return x.contiguous()


def _oracle(x, views):
    return torch.stack([_view(x, v) for v in views])


def _bits(t):
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _placed(x, lead):
    """x on the device, its first element `lead` elements behind a 256-byte boundary."""
    flat = torch.zeros(lead + x.numel(), dtype=x.dtype, device="cuda")
    view = flat[lead:].view(x.shape)
    view.copy_(x)
    return view


def _guard(dtype):
    return GUARD_U8 if dtype == torch.uint8 else GUARD_F32


def _out_buffer(shape, dtype, lead):
    """(flat, view): a device buffer of 64 guard elements, `lead` more, the output, and 80 guard elements behind."""
    numel = 1
    for d in shape:
        numel *= int(d)
    flat = torch.full((64 + lead + numel + 80,), _guard(dtype), dtype=dtype, device="cuda")
    return flat, flat[64 + lead:64 + lead + numel].view(*shape)


def _guards_intact(flat, numel, lead):
    f = flat.cpu()
    g = _guard(flat.dtype)
    return bool((f[:64 + lead] == g).all()) and bool((f[64 + lead + numel:] == g).all())


def _view_lists(h, w):
    codes = DIHEDRAL if h == w else FLIP
    lists = [(v,) for v in codes] + [FLIP]
    if h == w:
        lists += [DIHEDRAL, (5, 0, 5, 6)]
    else:
        lists += [(2, 1, 2)]
    return lists


# beyond the grid: one-byte pixels past their 128-pixel tile (square and not), and float32 / three-byte pixels past several
BIG = [(2, 130, 130, 1, True), (1, 129, 201, 1, True), (1, 131, 67, 3, True), (1, 70, 99, 1, False)]


@pytest.mark.parametrize("n,h,w,c,u8", CASES + BIG,
                         ids=IDS + [f"{n}x{h}x{w}x{c}-{'u8nhwc' if u8 else 'f32nchw'}" for n, h, w, c, u8 in BIG])
def test_views_bit_exact_against_torch(n, h, w, c, u8):
    from sykepic_hip import ops
    x = _batch(n, h, w, c, u8, 100 * n + 10 * h + c)
    in_lead = (3, 0, 5, 13)[(n + h) % 4] if u8 else (1, 0, 3, 13)[(n + h) % 4]
    xd = _placed(x, in_lead)
    for li, views in enumerate(_view_lists(h, w)):
        lead = ((0, 1, 7, 13) if u8 else (0, 1, 2, 3, 13))[(li + n) % (4 if u8 else 5)]
        flat, out = _out_buffer((len(views),) + tuple(x.shape), x.dtype, lead)
        got = ops.tta_views(xd, views, out=out)
        assert got is out
        what = f"views {views} output lead {lead} input lead {in_lead}"
        assert torch.equal(_bits(out.cpu()), _bits(_oracle(x, views))), what
        assert _guards_intact(flat, out.numel(), lead), f"{what}: memory around the output was written"
    assert torch.equal(_bits(xd.cpu()), _bits(x)), "the input batch was written"
    # two identical calls: identical bits
    views = DIHEDRAL if h == w else FLIP
    a, b = ops.tta_views(xd, views), ops.tta_views(xd, views)
    assert a.shape == (len(views),) + tuple(x.shape) and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape", [(2, 1, 7, 9), (5, 3, 33, 33), (2, 3, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_views_copy_every_float32_bit_pattern(shape):
    """No arithmetic touches an element: -0.0, denormals, infinities and a NaN payload arrive bit for bit."""
    from sykepic_hip import ops
    n, c, h, w = shape
    x = _batch(n, h, w, c, False, 5)
    special = torch.tensor([-0.0, 1e-40, -1e-42, 1.4e-45, float("inf"), float("-inf"), 3.4e38], dtype=torch.float32)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=_gen(9))[:4 * special.numel()]
    flat[idx] = special.repeat(4)
    bits = x.view(torch.int32).clone()
    bits.view(-1)[int(idx[0])] = 0x7FC12345                    # a NaN with a payload
    bits.view(-1)[int(idx[1])] = -0x003EDCBB                   # 0xFFC12345: a negative one
    x = bits.view(torch.float32)
    views = DIHEDRAL if h == w else FLIP
    out = ops.tta_views(x.cuda(), views)
    want = _oracle(x, views)
    assert torch.equal(_bits(out.cpu()), _bits(want))
    assert int((_bits(want) == 0x7FC12345).sum()) == len(views)


def test_views_image_sized_batch_all_eight_in_one_call():
    """2 x 180 x 180 x 3 (the loader's batch layout) and its float32 NCHW counterpart; one-byte pixels too, whose
    128-pixel tile the image straddles."""
    from sykepic_hip import ops
    for u8, c in ((True, 3), (False, 3), (True, 1)):
        x = _batch(2, 180, 180, c, u8, 77)
        out = ops.tta_views(x.cuda(), DIHEDRAL)
        assert torch.equal(_bits(out.cpu()), _bits(_oracle(x, DIHEDRAL))), (u8, c)


def test_views_refused_calls_on_device_tensors():
    from sykepic_hip import ops
    x = _batch(2, 8, 6, 3, True, 1).cuda()
    with pytest.raises(RuntimeError, match="h == w"):
        ops.tta_views(x, (0, 5))
    with pytest.raises(RuntimeError, match="0..7"):
        ops.tta_views(x, (0, 8))
    with pytest.raises(RuntimeError, match="k outside"):
        ops.tta_views(x, (0, 1, 2, 3, 0, 1, 2, 3, 0))
    with pytest.raises(RuntimeError, match="spk_tta_views"):     # (an empty output tensor has no address: null pointer)
        ops.tta_views(x, ())
    with pytest.raises(RuntimeError, match="overlap"):
        ops.tta_views(x, (1,), out=x.view((1,) + tuple(x.shape)))
    p = torch.zeros((3, 10), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):
        ops.tta_mean(p, out=p[2])


# ---- the mean ----
KS = [1, 2, 3, 4, 8]
NUMELS = [1, 50, 150, 1027]


def _probs(k, numel, seed):
    """[k, numel] float32: softmax rows of 50 classes where they fit, then values of mixed magnitude and sign (whose
    float32 sum depends on the order of the adds)."""
    g = _gen(seed)
    p = torch.empty((k, numel), dtype=torch.float32)
    rows = numel // 50
    if rows:
        p[:, :rows * 50] = torch.softmax(torch.randn((k, rows, 50), generator=g) * 3, dim=2).reshape(k, rows * 50)
    rest = numel - rows * 50
    if rest:
        mag = 10.0 ** torch.randint(-6, 7, (k, rest), generator=g).float()
        p[:, rows * 50:] = torch.randn((k, rest), generator=g) * mag
        if k >= 3:    # one element that leaves nothing to chance: 1e8 - 1e8 + 0 ... + 1 is 1 in view order, 0 reversed
            p[:, rows * 50] = 0.0
            p[0, rows * 50], p[1, rows * 50], p[k - 1, rows * 50] = 1e8, -1e8, 1.0
    return p


def _mean_oracle(p, order):
    s = p[order[0]].clone()
    for j in order[1:]:
        s = s + p[j]                      # one float32 add per view, in this order
    return s / torch.tensor(float(p.shape[0]), dtype=torch.float32)


@pytest.mark.parametrize("numel", NUMELS)
@pytest.mark.parametrize("k", KS)
def test_mean_bit_exact_and_in_view_order(k, numel):
    from sykepic_hip import ops
    p = _probs(k, numel, 31 * k + numel)
    want = _mean_oracle(p, list(range(k)))
    if k >= 3:
        rev = _mean_oracle(p, list(range(k))[::-1])
        assert not torch.equal(_bits(rev), _bits(want)), "the inputs do not tell the summation orders apart"
    for in_lead, lead in ((0, 0), (1, 3), (2, 1), (3, 2), (13, 13)):
        pd = _placed(p, in_lead)
        flat, out = _out_buffer((numel,), torch.float32, lead)
        got = ops.tta_mean(pd, out=out)
        assert got is out
        assert torch.equal(_bits(out.cpu()), _bits(want)), (in_lead, lead)
        assert _guards_intact(flat, numel, lead), "memory around the output was written"
        assert torch.equal(_bits(pd.cpu()), _bits(p)), "the input was written"
    # [k, n, classes] in, [n, classes] out; two identical calls: identical bits
    if numel % 50 == 0:
        pd = p.view(k, numel // 50, 50).cuda()
        a, b = ops.tta_mean(pd), ops.tta_mean(pd)
        assert a.shape == (numel // 50, 50) and torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(a.cpu().view(-1)), _bits(want))
