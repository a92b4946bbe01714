"""Single-operator test hooks of the C-ABI (``spk_op_*`` in include/sykepic_hip.h) on torch device tensors.

Each call runs exactly the launches ``spk_train_forward_backward`` makes for ONE Conv2d + BatchNorm2d layer
(the reference reaches them through ``net(x)`` / ``loss.backward()``, sykepic/train/train.py:240,242), so a
parity test can feed a kernel known operands.  Tensor conventions: activations and gradients are torch
``bfloat16`` tensors in NCHW *logical* shape; they are handed to the library as NHWC (``channels_last``
storage), weights as float32 OIHW (handed over as [Cout][kh][kw][Cin]).  No CPU fallback.
"""

import contextlib
import ctypes as C

import torch

from . import lib


def _nhwc(t):
    """NCHW logical tensor -> contiguous [N,H,W,C] bf16 device tensor."""
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _is_stem(cin, cout, k, stride, pad):
    return cin <= 4 and k == 7 and stride == 2 and pad == 3 and cout == 64


def _stem_input(x, dtype=torch.bfloat16):
    """[N,C<=4,H,W] -> NHWC with 4 stored channels and an even width (the layout spk_launch_to_nhwc4 produces)."""
    n, c, h, w = x.shape
    wp = (w + 1) & ~1
    out = torch.zeros((n, h, wp, 4), dtype=dtype, device=x.device)
    out[:, :, :w, :c] = x.permute(0, 2, 3, 1)
    return out


def conv_bn_train_forward(x, weight, gamma, beta, running_mean, running_var, res=None, relu=True, stride=1, pad=0):
    """Returns dict(out, raw, mask, mean, invstd); running_mean / running_var (float32 device tensors) are updated
    in place."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout, _, k, _ = weight.shape
    stem = _is_stem(cin, cout, k, stride, pad)
    xh = _stem_input(x) if stem else _nhwc(x.to(torch.bfloat16))
    wk = weight.float().permute(0, 2, 3, 1).contiguous()
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    # poison: every element must be written by the launches
    out = torch.full((n, oh, ow, cout), float("nan"), dtype=torch.bfloat16, device=dev)
    raw = torch.full_like(out, float("nan"))
    mask = torch.zeros((n * oh * ow, cout // 8), dtype=torch.uint8, device=dev)
    stats = torch.empty((2, cout), dtype=torch.float32, device=dev)
    resh = _nhwc(res.to(torch.bfloat16)) if res is not None else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv_bn_train_forward(
            _p(xh), _p(wk), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(resh), _p(out), _p(raw),
            _p(mask), _p(stats), n, h, w, cin, cout, k, stride, pad, int(bool(relu)), _stream(dev)))
    return {"out": _nchw(out), "raw": _nchw(raw), "mask": mask, "mean": stats[0], "invstd": stats[1]}


def bn_backward(g, mask, raw, mean, invstd, gamma, relu=True, g_res=None, res_accumulate=False, want_res=False):
    """g, raw: [N,C,H,W] bf16.  Returns dict(dy, dgamma, dbeta, g_res)."""
    so = lib.load()
    dev = g.device
    n, c, h, w = g.shape
    gh, rh = _nhwc(g), _nhwc(raw)
    dy = torch.empty_like(gh)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    gres = None
    if want_res or g_res is not None:
        gres = _nhwc(g_res.to(torch.bfloat16)) if g_res is not None else torch.empty_like(gh)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_bn_backward(_p(gh), _p(mask), _p(rh), _p(mean), _p(invstd), _p(gamma), _p(dgamma),
                                        _p(dbeta), _p(dy), _p(gres), int(bool(res_accumulate)), n * h * w, c,
                                        int(bool(relu)), _stream(dev)))
    return {"dy": _nchw(dy), "dgamma": dgamma, "dbeta": dbeta, "g_res": _nchw(gres) if gres is not None else None}


def conv_dgrad(dy, weight, in_hw, stride=1, pad=0, accumulate_into=None):
    """dx [N,Cin,H,W] bf16 = conv_transpose(dy, weight) (+ accumulate_into)."""
    so = lib.load()
    dev = dy.device
    n, cout = dy.shape[:2]
    _, cin, k, _ = weight.shape
    h, w = in_hw
    dyh = _nhwc(dy.to(torch.bfloat16))
    wk = weight.float().permute(0, 2, 3, 1).contiguous()
    if accumulate_into is not None:
        dx = _nhwc(accumulate_into.to(torch.bfloat16))
    else:
        # poison: every element must be written (or zeroed) by the launches
        dx = torch.full((n, h, w, cin), float("nan"), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv_dgrad(_p(dyh), _p(wk), _p(dx), int(accumulate_into is not None), n, h, w, cin, cout,
                                       k, stride, pad, _stream(dev)))
    return _nchw(dx)


def conv_dgrad_bn_backward(dy, weight, in_hw, raw, mask, mean, invstd, gamma, pad=0, relu=True, accumulate_into=None,
                           res_src=None, res_bits=None):
    """Stride-1 data gradient whose epilogue also makes the BatchNorm-backward sums of the layer that produced the conv's
    input, then that layer's finalize + apply (spk_op_conv_dgrad_bn_backward).  raw [N,Cin,H,W] bf16, mask as returned by
    `conv_bn_train_forward`.  res_src [N,Cin,H,W] bf16 + res_bits (instead of accumulate_into): the shortcut gradient
    res_src * bit added at its source.  Returns dict(g, dy, dgamma, dbeta): g = the stored input gradient."""
    so = lib.load()
    dev = dy.device
    n, cout = dy.shape[:2]
    _, cin, k, _ = weight.shape
    h, w = in_hw
    dyh = _nhwc(dy.to(torch.bfloat16))
    wk = weight.float().permute(0, 2, 3, 1).contiguous()
    if accumulate_into is not None:
        dx = _nhwc(accumulate_into.to(torch.bfloat16))
    else:
        dx = torch.full((n, h, w, cin), float("nan"), dtype=torch.bfloat16, device=dev)
    rawh = _nhwc(raw.to(torch.bfloat16))
    rsh = _nhwc(res_src.to(torch.bfloat16)) if res_src is not None else None
    dyp = torch.empty_like(rawh)
    dgamma = torch.empty(cin, dtype=torch.float32, device=dev)
    dbeta = torch.empty(cin, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv_dgrad_bn_backward(
            _p(dyh), _p(wk), _p(dx), int(accumulate_into is not None), _p(rawh), _p(mask), _p(mean), _p(invstd), _p(gamma),
            _p(dgamma), _p(dbeta), _p(dyp), n, h, w, cin, cout, k, pad, int(bool(relu)), _p(rsh), _p(res_bits), _stream(dev)))
    return {"g": _nchw(dx), "dy": _nchw(dyp), "dgamma": dgamma, "dbeta": dbeta}


@contextlib.contextmanager
def pinned_conv(cfg, dma, nbuf=-1):
    """Every implicit-GEMM convolution inside the block runs tile config `cfg` with main-loop flavour `dma`, every weight
    gradient `nbuf` LDS stages (spk_op_conv_pin; -1: the tuner decides).  A flavour that the tile does not instantiate
    makes the hooks raise RuntimeError "does not fit".  The pin is process-wide and is lifted on exit, however the block
    ends."""
    so = lib.load()
    lib.check(so.spk_op_conv_pin(int(cfg), int(dma), int(nbuf)))
    try:
        yield
    finally:
        lib.check(so.spk_op_conv_pin(-1, -1, -1))


def conv_wgrad(x, dy, k, stride=1, pad=0):
    """dw [Cout,Cin,k,k] float32 from x [N,Cin,H,W] and dy [N,Cout,Ho,Wo] (bf16)."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    stem = _is_stem(cin, cout, k, stride, pad)
    xh = _stem_input(x.to(torch.bfloat16)) if stem else _nhwc(x.to(torch.bfloat16))
    dyh = _nhwc(dy.to(torch.bfloat16))
    dw = torch.full((cout, k, k, cin), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv_wgrad(_p(xh), _p(dyh), _p(dw), n, h, w, cin, cout, k, stride, pad, _stream(dev)))
    return dw.permute(0, 3, 1, 2)


def pw_fp8(x, weight, bn_scale, bn_bias, act=0, a_scale=1.0, y_scale=1.0, out_fp8=False, res=None, gate=None, hw=1):
    """fp8 pointwise conv (spk_op_pw_fp8).  x: [M, cin] float16, or uint8 holding e4m3 bytes (value = byte *
    a_scale); weight [cout, cin] float32; returns [M, cout] float16, or uint8 e4m3 bytes when out_fp8."""
    so = lib.load()
    dev = x.device
    m, cin = x.shape
    cout = weight.shape[0]
    a_fp8 = x.dtype == torch.uint8
    x = x.contiguous()
    y = torch.empty((m, cout), dtype=torch.uint8 if out_fp8 else torch.float16, device=dev)
    w = weight.float().contiguous()
    with torch.cuda.device(dev):
        lib.check(so.spk_op_pw_fp8(_p(x), int(a_fp8), _p(w), _p(y), int(bool(out_fp8)),
                                   _p(res.contiguous()) if res is not None else None, _p(bn_scale.float().contiguous()),
                                   _p(bn_bias.float().contiguous()),
                                   _p(gate.float().contiguous()) if gate is not None else None, int(hw), m, cin, cout,
                                   int(act), float(a_scale), float(y_scale), _stream(dev)))
    return y


def dwconv(x, weight, bn_scale, bn_bias, k, stride=1, act=2, lds=1):
    """Depthwise conv + folded BN + activation (spk_op_dwconv).  x [N,C,H,W] float16, weight [C,1,k,k];
    returns (y [N,C,Ho,Wo] float16, pool [N,C] float32 sums of y before rounding)."""
    so = lib.load()
    dev = x.device
    n, c, h, w = x.shape
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, ho, wo, c), float("nan"), dtype=torch.float16, device=dev)
    pool = torch.empty((n, c), dtype=torch.float32, device=dev)
    wk = weight.float().reshape(c, k * k).contiguous()
    with torch.cuda.device(dev):
        lib.check(so.spk_op_dwconv(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                   _p(y), _p(pool), n, h, w, c, k, stride, int(act), int(lds), _stream(dev)))
    return y.permute(0, 3, 1, 2), pool


def conv1x1_num_configs():
    return int(lib.load().spk_op_conv1x1_num_configs())


def conv1x1(x, weight, bn_scale, bn_bias, stride=1, relu=True, res=None, split=True, cfg=0):
    """Eval-path 1x1 conv + folded BN (+ shortcut) (+ ReLU) (spk_op_conv1x1).  x [N,Cin,H,W] float16, weight
    [Cout,Cin] (or [Cout,Cin,1,1]); res [N,Cout,Ho,Wo] float16 or None.  cfg >= 0: that configuration of the
    direct-operand kernel (raises RuntimeError "does not fit" when it cannot run the problem), cfg < 0: the implicit
    GEMM.  Returns [N,Cout,Ho,Wo] float16."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    rh = res.half().permute(0, 2, 3, 1).contiguous() if res is not None else None
    y = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.float16, device=dev)
    wk = weight.float().reshape(cout, cin).contiguous()
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv1x1(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                    _p(rh) if rh is not None else None, _p(y), n, h, w, cin, cout, int(stride),
                                    int(bool(relu)), int(bool(split)), int(cfg), _stream(dev)))
    return y.permute(0, 3, 1, 2)


def conv1x1_chain(x, weight, bn_scale, bn_bias, res, weight_z, bnz_scale, bnz_bias, relu=True, relu_z=True):
    """Two chained 1x1 convs in one launch (spk_op_conv1x1_chain): returns (y [N,256,H,W], z [N,Coutz,H,W]) float16."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout, coutz = weight.shape[0], weight_z.shape[0]
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    rh = res.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.float16, device=dev)
    z = torch.full((n, h, w, coutz), float("nan"), dtype=torch.float16, device=dev)
    f = lambda t: t.float().contiguous()   # noqa: E731
    wk, wzk = f(weight.reshape(cout, cin)), f(weight_z.reshape(coutz, cout))
    s1, b1, s2, b2 = f(bn_scale), f(bn_bias), f(bnz_scale), f(bnz_bias)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv1x1_chain(_p(xh), _p(wk), _p(s1), _p(b1), _p(rh), _p(y), _p(wzk), _p(s2), _p(b2), _p(z), n, h, w,
                                          cin, cout, coutz, int(bool(relu)), int(bool(relu_z)), _stream(dev)))
    return y.permute(0, 3, 1, 2), z.permute(0, 3, 1, 2)


def conv1x1_dual(x, w1, bn1_scale, bn1_bias, x2, w2, bn2_scale, bn2_bias, stride2=2, relu=True, split=False, cfg=0):
    """A block-closing 1x1 conv and the block's 1x1 shortcut conv as one K-concatenated GEMM (spk_op_conv1x1_dual):
    act(BN1(W1 . x) + BN2(W2 . x2[::stride2, ::stride2])).  x [N,Cin,Ho,Wo], x2 [N,Cin2,H2,W2] float16; returns
    [N,Cout,Ho,Wo] float16.  Raises RuntimeError "does not fit" when `cfg` cannot run the problem."""
    so = lib.load()
    dev = x.device
    n, cin, ho, wo = x.shape
    _, cin2, h2, w2d = x2.shape
    cout = w1.shape[0]
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    x2h = x2.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.float16, device=dev)
    f = lambda t: t.float().contiguous()   # noqa: E731
    w1k, w2k = f(w1.reshape(cout, cin)), f(w2.reshape(cout, cin2))
    s1, b1, s2, b2 = f(bn1_scale), f(bn1_bias), f(bn2_scale), f(bn2_bias)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv1x1_dual(_p(xh), _p(w1k), _p(s1), _p(b1), _p(x2h), _p(w2k), _p(s2), _p(b2), _p(y), n, ho, wo,
                                         cin, h2, w2d, cin2, cout, int(stride2), int(bool(relu)), int(bool(split)), int(cfg),
                                         _stream(dev)))
    return y.permute(0, 3, 1, 2)


def conv3x3_num_configs():
    return int(lib.load().spk_op_conv3x3_num_configs())


def conv3x3(x, weight, bn_scale, bn_bias, relu=True, split=False, cfg=0, res=None):
    """Eval-path 3x3 stride-1 pad-1 conv + folded BN (+ shortcut) (+ ReLU) (spk_op_conv3x3).  x [N,Cin,H,W] float16,
    weight [Cout,Cin,3,3], res [N,Cout,H,W] or None; cfg >= 0: that configuration of the LDS-window kernel, cfg < 0: the
    implicit GEMM."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, h, w, cout), float("nan"), dtype=torch.float16, device=dev)
    wk = weight.float().permute(0, 2, 3, 1).contiguous()   # OIHW -> O,kh,kw,I
    rh = res.half().permute(0, 2, 3, 1).contiguous() if res is not None else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv3x3(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                    _p(rh) if rh is not None else None, _p(y), n, h, w, cin, cout, int(bool(relu)), int(bool(split)), int(cfg),
                                    _stream(dev)))
    return y.permute(0, 3, 1, 2)


def conv3x3_direct_num_configs():
    return int(lib.load().spk_op_conv3x3_direct_num_configs())


def conv3x3_direct(x, weight, bn_scale, bn_bias, relu=True, split=False, cfg=0, res=None, stride=1, iters=0):
    """Eval-path 3x3 pad-1 conv + folded BN (+ shortcut) (+ ReLU) by the direct 64 -> 64 kernel (spk_op_conv3x3_direct,
    csrc/conv_d3.hip).  x [N,Cin,H,W] float16, weight [Cout,Cin,3,3], res [N,Cout,Ho,Wo] or None.  cfg >= 0: that
    configuration, RuntimeError "does not fit" for a problem the kernel does not take; cfg < 0: the implicit GEMM on the
    same problem.  iters > 0: returns (y, mean milliseconds of one launch over iters back-to-back launches)."""
    import ctypes as C
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, ho, wo, cout), float("nan"), dtype=torch.float16, device=dev)
    wk = weight.float().permute(0, 2, 3, 1).contiguous()   # OIHW -> O,kh,kw,I
    rh = res.half().permute(0, 2, 3, 1).contiguous() if res is not None else None
    ms = C.c_float(0.0)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv3x3_direct(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                           _p(rh) if rh is not None else None, _p(y), n, h, w, cin, cout, int(stride),
                                           int(bool(relu)), int(bool(split)), int(cfg), int(iters), C.byref(ms), _stream(dev)))
    y = y.permute(0, 3, 1, 2)
    return (y, float(ms.value)) if iters > 0 else y


def bottleneck(x, w1, w2, w3, bn1, bn2, bn3, fused=True, iters=0, stamps=None, wz=None, bnz=None):
    """Eval-path identity bottleneck block (spk_op_bottleneck): x [N,4cm,H,W] float16, w1 [cm,4cm,1,1], w2 [cm,cm,3,3],
    w3 [4cm,cm,1,1], bn* = (scale, shift) of the folded eval BatchNorms.  fused: the one-kernel form (csrc/conv_bneck.hip),
    else the eval path's three launches.  Returns y [N,4cm,H,W] (and the mean milliseconds per block when iters > 0)."""
    import ctypes as C
    so = lib.load()
    dev = x.device
    n, c4, h, w = x.shape
    cm = w1.shape[0]
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    y = torch.full((n, h, w, c4), float("nan"), dtype=torch.float16, device=dev)
    k1 = w1.float().reshape(cm, c4).contiguous()
    k2 = w2.float().permute(0, 2, 3, 1).contiguous()
    k3 = w3.float().reshape(c4, cm).contiguous()
    vecs = [t.float().contiguous() for pair in (bn1, bn2, bn3) for t in pair]
    ms = C.c_float(0.0)
    # fused: False / 0 three launches, True / 1 the whole block as one kernel, 2 conv1 + (conv2 + conv3 + shortcut [+ wz]) kernel
    kz = z = sz = bz = None
    coutz = 0
    if wz is not None:      # the conv + BN + ReLU that reads the block's output (the next block's conv1): z comes back too
        coutz = wz.shape[0]
        kz = wz.float().reshape(coutz, c4).contiguous()
        sz, bz = (t.float().contiguous() for t in bnz)
        z = torch.full((n, h, w, coutz), float("nan"), dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_bottleneck(_p(xh), _p(k1), _p(k2), _p(k3), *[_p(v) for v in vecs], _p(y), n, h, w, cm,
                                       int(fused), int(iters), C.cast(C.pointer(ms), C.c_void_p), _stream(dev),
                                       _p(stamps) if stamps is not None else None,
                                       _p(kz) if kz is not None else None, _p(sz) if sz is not None else None,
                                       _p(bz) if bz is not None else None, _p(z) if z is not None else None, coutz))
    out = y.permute(0, 3, 1, 2)
    if z is not None:
        out = (out, z.permute(0, 3, 1, 2))
    return (out, float(ms.value)) if iters > 0 else out


def zero_sum_round(w, mu=None, period=None):
    """w [rows, row_len] float32 device tensor, mu [period] or None -> the zero-sum rounded rows (float32 values that are
    fp16 numbers), csrc/zero_sum.hip."""
    so = lib.load()
    w = w.float().contiguous()
    out = torch.empty_like(w)
    rows, row_len = w.shape
    if mu is not None:
        mu = mu.float().contiguous()
        period = period or mu.numel()
    with torch.cuda.device(w.device):
        lib.check(so.spk_op_zero_sum_round(_p(w), _p(mu), _p(out), rows, row_len, int(period or row_len), _stream(w.device)))
    return out


# ---- the MBConv training kernels (csrc/train_effnet.hip), one layer at a time.  Unlike the hooks above these take the
# step's own layout: bf16 NHWC device tensors whose last dimension is the PADDED channel count C (a multiple of 64, zeros
# in the pad channels); parameters float32 with c_log <= C entries.

def _bf16c(t):
    assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.is_cuda, "bf16 contiguous device tensor expected"
    return t


def _f32c(t):
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda, "float32 contiguous device tensor expected"
    return t


def mbconv_geometry(kind, m=0, c=0, hw=0, s=0):
    """spk_op_mbconv_geometry: the launch geometry the kernels of csrc/train_effnet.hip would get (no GPU needed).
    Returns the 8 integers (see include/sykepic_hip.h); raises RuntimeError when the launchers refuse the problem."""
    so = lib.load()
    out = (C.c_int * 8)()
    lib.check(so.spk_op_mbconv_geometry(int(kind), int(m), int(c), int(hw), int(s), out))
    return list(out)


def dw_train(x, weight, c_log, k, stride=1, pad=None, dy=None, want_y=True, want_dx=False, want_dw=False,
             accumulate_into=None):
    """Depthwise layer of a training step (spk_op_dw_train).  x [N,H,W,C] bf16, weight [c_log, k*k] float32, dy
    [N,Ho,Wo,C] bf16.  Returns dict(y, dx, dw): the raw forward output, the data gradient (added to `accumulate_into`
    [N,H,W,C] when given) and the weight gradient [c_log, k*k]; entries not asked for are None."""
    so = lib.load()
    dev = x.device
    n, h, w, c = x.shape
    pad = (k - 1) // 2 if pad is None else pad
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    wk = _f32c(weight.reshape(c_log, k * k))
    nan = float("nan")   # poison: every element must be written by the launches
    y = torch.full((n, ho, wo, c), nan, dtype=torch.bfloat16, device=dev) if want_y else None
    dx = None
    if accumulate_into is not None:
        dx = accumulate_into.clone()
    elif want_dx:
        dx = torch.full((n, h, w, c), nan, dtype=torch.bfloat16, device=dev)
    dw = torch.full((c_log, k * k), nan, dtype=torch.float32, device=dev) if want_dw else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_dw_train(_p(_bf16c(x)), _p(_bf16c(dy)) if dy is not None else None, _p(wk), _p(y), _p(dx),
                                     _p(dw), int(accumulate_into is not None), n, h, w, c, int(c_log), int(k),
                                     int(stride), int(pad), _stream(dev)))
    return {"y": y, "dx": dx, "dw": dw}


def bna_forward(raw, gamma, beta, running_mean, running_var, act=0, res=None, rowscale=None, pool=False, eps=1e-5,
                momentum=0.1):
    """BatchNorm (train mode) + activation forward (spk_op_bna_forward).  raw [N,HW,C] bf16; gamma / beta /
    running_* float32 [c_log] (the running statistics are updated in place); res [N,HW,C] bf16, rowscale [N] float32.
    pool: the form that also returns the per-chunk channel sums of the output, pool_part [N,chunks,C].
    Returns dict(out, st [4,C] = mean, invstd, scale, shift, pool_part)."""
    so = lib.load()
    dev = raw.device
    n, hw, c = raw.shape
    c_log = gamma.numel()
    out = torch.full((n, hw, c), float("nan"), dtype=torch.bfloat16, device=dev)
    st = torch.full((4, c), float("nan"), dtype=torch.float32, device=dev)
    part = None
    if pool:
        chunks = mbconv_geometry(2, c=c, hw=hw)[1]
        part = torch.full((n, chunks, c), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_bna_forward(_p(_bf16c(raw)), _p(_f32c(gamma)), _p(_f32c(beta)), _p(_f32c(running_mean)),
                                        _p(_f32c(running_var)), _p(_bf16c(res)) if res is not None else None,
                                        _p(_f32c(rowscale)), _p(out), _p(part), _p(st), n, hw, c, c_log, int(act),
                                        float(eps), float(momentum), _stream(dev)))
    return {"out": out, "st": st, "pool_part": part}


def bna_backward(g, raw, st, gamma, act=0, rowscale=None, g_res=None, want_res=False):
    """Its backward (spk_op_bna_backward).  g, raw [N,HW,C] bf16, st [4,C] as bna_forward returned it, gamma [c_log].
    g_res: the shortcut gradient accumulates into a copy of it; want_res: it is returned on its own.
    Returns dict(dy, dgamma, dbeta, g_res)."""
    so = lib.load()
    dev = g.device
    n, hw, c = g.shape
    c_log = gamma.numel()
    dy = torch.full((n, hw, c), float("nan"), dtype=torch.bfloat16, device=dev)
    dgamma = torch.full((c_log,), float("nan"), dtype=torch.float32, device=dev)
    dbeta = torch.full((c_log,), float("nan"), dtype=torch.float32, device=dev)
    gres = None
    if g_res is not None:
        gres = g_res.clone()
    elif want_res:
        gres = torch.full((n, hw, c), float("nan"), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_bna_backward(_p(_bf16c(g)), _p(_bf16c(raw)), _p(_f32c(st)), _p(_f32c(gamma)),
                                         _p(_f32c(rowscale)), _p(dy), _p(dgamma), _p(dbeta), _p(gres),
                                         int(g_res is not None), n, hw, c, c_log, int(act), _stream(dev)))
    return {"dy": dy, "dgamma": dgamma, "dbeta": dbeta, "g_res": gres}


def se_train_forward(a, w1, b1, w2, b2, gate_kind=0, pool_part=None, want_out=True):
    """Squeeze-excitation forward (spk_op_se_train_forward).  a [N,HW,C] bf16; w1 [S,Cl], b1 [S], w2 [Cl,S], b2 [Cl]
    float32; pool_part [N,chunks,C]: the sums bna_forward(pool=True) left, instead of pooling `a`.
    Returns dict(pooled [N,C], u1 [N,S], h1 [N,S], gate [N,C], out [N,HW,C])."""
    so = lib.load()
    dev = a.device
    n, hw, c = a.shape
    s_hid, cl = w1.shape
    nan = float("nan")
    pooled = torch.full((n, c), nan, dtype=torch.float32, device=dev)
    gate = torch.full((n, c), nan, dtype=torch.float32, device=dev)
    u1 = torch.full((n, s_hid), nan, dtype=torch.float32, device=dev)
    h1 = torch.full((n, s_hid), nan, dtype=torch.float32, device=dev)
    out = torch.full((n, hw, c), nan, dtype=torch.bfloat16, device=dev) if want_out else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_se_train_forward(_p(_bf16c(a)), _p(_f32c(pool_part)), _p(_f32c(w1)), _p(_f32c(b1)),
                                             _p(_f32c(w2)), _p(_f32c(b2)), _p(pooled), _p(u1), _p(h1), _p(gate), _p(out),
                                             n, hw, c, cl, s_hid, int(gate_kind), _stream(dev)))
    return {"pooled": pooled, "u1": u1, "h1": h1, "gate": gate, "out": out}


def se_train_backward(g, a, saved, w1, w2, gate_kind=0):
    """Its backward (spk_op_se_train_backward).  g, a [N,HW,C] bf16, saved: what se_train_forward returned.
    Returns dict(da, gw1, gb1, gw2, gb2, du2 [N,C], du1 [N,S], pool_part [N,chunks,C] = per-chunk sums of g * a)."""
    so = lib.load()
    dev = g.device
    n, hw, c = g.shape
    s_hid, cl = w1.shape
    nan = float("nan")
    f = lambda *shape: torch.full(shape, nan, dtype=torch.float32, device=dev)   # noqa: E731
    du2, du1 = f(n, c), f(n, s_hid)
    part = f(n, mbconv_geometry(2, c=c, hw=hw)[1], c)
    gw1, gb1, gw2, gb2 = f(s_hid, cl), f(s_hid), f(cl, s_hid), f(cl)
    da = torch.full((n, hw, c), nan, dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_se_train_backward(
            _p(_bf16c(g)), _p(_bf16c(a)), _p(_f32c(saved["gate"])), _p(_f32c(saved["u1"])), _p(_f32c(saved["h1"])),
            _p(_f32c(saved["pooled"])), _p(_f32c(w1)), _p(_f32c(w2)), _p(du2), _p(du1), _p(part), _p(da), _p(gw1), _p(gb1),
            _p(gw2), _p(gb2), n, hw, c, cl, s_hid, int(gate_kind), _stream(dev)))
    return {"da": da, "gw1": gw1, "gb1": gb1, "gw2": gw2, "gb2": gb2, "du2": du2, "du1": du1, "pool_part": part}


def se_wgrad(du2, h1, du1, pooled, cl):
    """The parameter-gradient kernel of the squeeze-excitation layer alone, on the caller's vectors
    (spk_op_se_train_backward with g == NULL): du2, pooled [N,C], h1, du1 [N,S] float32.
    Returns dict(gw1 [S,cl], gb1 [S], gw2 [cl,S], gb2 [cl])."""
    so = lib.load()
    dev = du2.device
    n, c = du2.shape
    s_hid = h1.shape[1]
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
    gw1, gb1, gw2, gb2 = f(s_hid, cl), f(s_hid), f(cl, s_hid), f(cl)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_se_train_backward(None, None, None, None, _p(_f32c(h1)), _p(_f32c(pooled)), None, None,
                                              _p(_f32c(du2)), _p(_f32c(du1)), None, None, _p(gw1), _p(gb1), _p(gw2),
                                              _p(gb2), n, 1, c, int(cl), s_hid, 0, _stream(dev)))
    return {"gw1": gw1, "gb1": gb1, "gw2": gw2, "gb2": gb2}


def stem3_train(x4, weight, c, dy=None, w_in=None):
    """The 3x3 stride-2 stem of a training step (spk_op_stem3_train).  x4 [N,H,Wp,4] bf16: pixel values x 255 in the
    first cin channels, Wp = the width rounded up to even (`w_in`: the logical width, default Wp); weight [cout,9,cin]
    float32; dy [N,Ho,Wo,C] bf16.  Returns dict(y [N,Ho,Wo,C] raw output, dw [cout,9,cin] or None)."""
    so = lib.load()
    dev = x4.device
    n, h, wp, _ = x4.shape
    w = wp if w_in is None else w_in
    assert wp == (w + 1) & ~1
    cout, _, cin = weight.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.full((n, ho, wo, c), float("nan"), dtype=torch.bfloat16, device=dev)
    dw = torch.full((cout, 9, cin), float("nan"), dtype=torch.float32, device=dev) if dy is not None else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_stem3_train(_p(_bf16c(x4)), _p(_f32c(weight)), _p(_bf16c(dy)) if dy is not None else None,
                                        _p(y), _p(dw), n, h, w, cin, cout, int(c), _stream(dev)))
    return {"y": y, "dw": dw}


# ---- the MBConv eval kernels and the eval stems (csrc/conv_igemm.hip PADC / GATE, effnet.hip, conv_stem.hip), one layer
# at a time.  Every output is NaN-poisoned and allocated with a sentinel tail of at least one more pixel row, which the
# launches must leave alone (AssertionError otherwise).
SENTINEL = -1234.0


def _guarded(shape, dtype, dev, tail):
    """(flat buffer of numel + tail elements, view of its first numel elements as `shape`): NaN, then the sentinel."""
    numel = 1
    for d in shape:
        numel *= int(d)
    buf = torch.full((numel + int(tail),), float("nan"), dtype=dtype, device=dev)
    buf[numel:] = SENTINEL
    return buf, buf[:numel].view(*shape)


def _check_tail(buf, numel, what):
    tail = buf[numel:]
    if not bool((tail == SENTINEL).all()):
        bad = int((tail != SENTINEL).nonzero()[0])
        raise AssertionError(f"{what}: element {bad} behind the end of the output was written ({float(tail[bad])})")


def mbconv_eval_geometry(kind, a=0, b=0, c=0, d=0):
    """spk_op_mbconv_eval_geometry: what the launchers of the eval kernels below choose (no GPU needed).  Returns the 8
    integers (see include/sykepic_hip.h)."""
    so = lib.load()
    out = (C.c_int * 8)()
    lib.check(so.spk_op_mbconv_eval_geometry(int(kind), int(a), int(b), int(c), int(d), out))
    return list(out)


def conv1x1_padded(x, weight, bn_scale, bn_bias, act=0, res=None, gate=None, split=False):
    """Eval-path 1x1 conv + folded BN (+ shortcut) + activation on channel counts that are multiples of 8 only
    (spk_op_conv1x1_padded: spk_launch_pack_padded + the implicit GEMM with cin_s / cout_s).  x [N,Cin,H,W] float16,
    weight [Cout,Cin], res [N,Cout,H,W] float16 or None, gate [N,Cin] float32 or None (the squeeze-excitation gates,
    multiplied into the operand: spk_set_gate).  act: 0 none, 1 ReLU, 2 SiLU, 3 Hardswish.  Honours `pinned_conv`.
    Returns [N,Cout,H,W] float16."""
    so = lib.load()
    dev = x.device
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    xh = x.half().permute(0, 2, 3, 1).contiguous()
    rh = res.half().permute(0, 2, 3, 1).contiguous() if res is not None else None
    gh = gate.float().contiguous() if gate is not None else None
    # (a pixel row, and no less than the 64-channel GEMM tile that a missing column check would store)
    buf, y = _guarded((n, h, w, cout), torch.float16, dev, max(w * cout, 64))
    wk = weight.float().reshape(cout, cin).contiguous()
    with torch.cuda.device(dev):
        lib.check(so.spk_op_conv1x1_padded(_p(xh), _p(wk), _p(bn_scale.float().contiguous()),
                                           _p(bn_bias.float().contiguous()), _p(rh), _p(gh), _p(buf), n, h, w, cin, cout,
                                           int(act), int(bool(split)), _stream(dev)))
    _check_tail(buf, y.numel(), "conv1x1_padded y")
    return y.permute(0, 3, 1, 2)


def se_eval(partial, w1, b1, w2, b2, hw, gate_kind=0, x=None):
    """Eval squeeze-excitation (spk_op_se_eval: spk_launch_se) from the pool partials [N,chunks,C] float32 (sums over
    the hw pixels).  w1 [S,C], b1 [S], w2 [C,S], b2 [C] float32; x [N,hw,C] float16 or None (the gates only).
    Returns dict(hid [N,S], scale [N,C] float32, y [N,hw,C] float16 or None)."""
    so = lib.load()
    dev = partial.device
    n, chunks, c = partial.shape
    sq = w1.shape[0]
    # one buffer: the gates, the hidden vector directly behind them (the layout of the model's scratch), the sentinel
    buf = torch.full((n * c + n * sq + max(c, sq),), float("nan"), dtype=torch.float32, device=dev)
    buf[n * c + n * sq:] = SENTINEL
    scale, hid = buf[:n * c].view(n, c), buf[n * c:n * c + n * sq].view(n, sq)
    ybuf = y = xh = None
    if x is not None:
        xh = x.half().contiguous()
        assert xh.shape == (n, hw, c)
        ybuf, y = _guarded((n, hw, c), torch.float16, dev, max(c, 8))
    with torch.cuda.device(dev):
        lib.check(so.spk_op_se_eval(_p(xh), _p(_f32c(partial)), chunks, _p(_f32c(w1)), _p(_f32c(b1)), _p(_f32c(w2)),
                                    _p(_f32c(b2)), _p(hid), _p(scale), _p(ybuf), n, int(hw), c, sq, int(gate_kind),
                                    _stream(dev)))
    _check_tail(buf, n * c + n * sq, "se_eval scale / hid")
    if y is not None:
        _check_tail(ybuf, y.numel(), "se_eval y")
    return {"hid": hid, "scale": scale, "y": y}


def _stem_eval_input(x):
    """Images [N,3,H,W] on the k / 255 grid in [0, 1] -> the fp16 NHWC4, even-width, x 255 tensor the model builds."""
    k = torch.round(x.double() * 255.0)
    assert float((x.double() * 255.0 - k).abs().max()) < 1e-3 and float(k.min()) >= 0 and float(k.max()) <= 255, \
        "pixel values must be k / 255"
    return _stem_input(k.to(torch.float16), torch.float16)


def stem3_eval(x, weight, bn_scale, bn_bias, act=2):
    """The 3x3/2 RGB stem of the eval path (spk_op_stem3_eval: pack_stem3 + spk_launch_stem3x3).  x [N,3,H,W] on the
    k / 255 grid, weight [Cout,3,3,3] (OIHW), ordinary folded-BN scale / shift (1 / 255 is folded into the scale inside,
    where the model does it).  Returns [N,Cout,Ho,Wo] float16."""
    so = lib.load()
    dev = x.device
    n, _, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xh = _stem_eval_input(x)
    wk = weight.float().permute(0, 2, 3, 1).contiguous()
    # (a pixel row, and no less than the four outputs a thread of the kernel owns)
    buf, y = _guarded((n, ho, wo, cout), torch.float16, dev, max(wo, 4) * cout)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_stem3_eval(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                       _p(buf), n, h, w, cout, int(act), _stream(dev)))
    _check_tail(buf, y.numel(), "stem3_eval y")
    return y.permute(0, 3, 1, 2)


def stem7_eval(x, weight, bn_scale, bn_bias, split=False, pool=False):
    """The 7x7/2 ResNet stem + ReLU of the eval path (spk_op_stem7_eval: spk_launch_pack_weights(CONV_MODE_STEM) +
    spk_conv_launch).  x [N,3,H,W] on the k / 255 grid, weight [64,3,7,7].  pool: the kernel variant with the fused 3x3/2
    max-pool, which writes only the pooled tensor.  Returns [N,64,Ho,Wo] (pool: [N,64,(Ho-1)//2+1,(Wo-1)//2+1]) float16."""
    so = lib.load()
    dev = x.device
    n, _, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if pool:
        ho, wo = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    xh = _stem_eval_input(x)
    wk = weight.float().permute(0, 2, 3, 1).contiguous()
    buf, y = _guarded((n, ho, wo, 64), torch.float16, dev, wo * 64)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_stem7_eval(_p(xh), _p(wk), _p(bn_scale.float().contiguous()), _p(bn_bias.float().contiguous()),
                                       None if pool else _p(buf), _p(buf) if pool else None, n, h, w, int(bool(split)),
                                       _stream(dev)))
    _check_tail(buf, y.numel(), "stem7_eval y")
    return y.permute(0, 3, 1, 2)


# ---- the classifier head, the loss and the pooling layers (csrc/head.hip, pointwise.hip, train_kernels.hip) ----
def _h16c(t):
    assert t.dtype in (torch.bfloat16, torch.float16) and t.is_contiguous() and t.is_cuda, \
        "bf16 / fp16 contiguous device tensor expected"
    return t


def linear(x, w, b=None):
    """y [N,out] = x [N,in] . w [out,in]^T + b (spk_op_linear: the launch of `spk_launch_linear_fwd`)."""
    so = lib.load()
    dev = x.device
    n, fin = x.shape
    fout = w.shape[0]
    y = torch.full((n, fout), float("nan"), dtype=torch.float32, device=dev)   # poison: every element must be written
    with torch.cuda.device(dev):
        lib.check(so.spk_op_linear(_p(_f32c(x)), _p(_f32c(w)), _p(_f32c(b)), _p(y), n, fin, fout, _stream(dev)))
    return y


def linear_backward(gy, x, w, dw=None, db=None, dx=None, form=-1):
    """The Linear layer's backward as a training step runs it (spk_op_linear_backward), into the caller's float32
    buffers dw [out,in], db [out], dx [N,in]; None skips that gradient.  form: -1 production's GEMM, 0 MFMA, 1 FMA."""
    so = lib.load()
    dev = gy.device
    n, fout = gy.shape
    fin = x.shape[1] if x is not None else w.shape[1]
    with torch.cuda.device(dev):
        lib.check(so.spk_op_linear_backward(_p(_f32c(gy)), _p(_f32c(x)), _p(_f32c(w)), _p(_f32c(dw)), _p(_f32c(db)),
                                            _p(_f32c(dx)), n, fin, fout, int(form), _stream(dev)))


def softmax(z, base):
    """p = softmax(z * log(base)) per row (spk_op_softmax)."""
    so = lib.load()
    dev = z.device
    n, c = z.shape
    p = torch.full((n, c), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_softmax(_p(_f32c(z)), _p(p), n, c, float(base), _stream(dev)))
    return p


def cross_entropy(z, labels, stats, dz=None):
    """spk_op_cross_entropy: adds (sum of the row losses, correct rows) to stats [2] float32 and writes dz [N,c] (the
    caller's buffer; None: no gradient)."""
    so = lib.load()
    dev = z.device
    n, c = z.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.is_cuda and labels.numel() == n
    with torch.cuda.device(dev):
        lib.check(so.spk_op_cross_entropy(_p(_f32c(z)), _p(labels), n, c, _p(_f32c(stats)), _p(_f32c(dz)), _stream(dev)))


def cross_entropy_ex(z, labels, stats, weight=None, label_smoothing=0.0, counts=None, dz=None):
    """spk_op_cross_entropy_ex: CrossEntropyLoss(weight, label_smoothing).  Adds (n * loss, correct rows) to stats [2]
    float32 and per class (rows, correct rows) to counts [c, 2] int32 (None: no counters); writes dz [N,c] (the caller's
    buffer; None: no gradient).  weight: float32 [c] on the device or None (all ones)."""
    so = lib.load()
    dev = z.device
    n, c = z.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.is_cuda and labels.numel() == n
    assert weight is None or weight.numel() == c
    assert counts is None or (counts.dtype == torch.int32 and counts.is_contiguous() and counts.is_cuda
                              and counts.numel() == 2 * c)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_cross_entropy_ex(_p(_f32c(z)), _p(labels), n, c, _p(_f32c(weight)), float(label_smoothing),
                                             _p(_f32c(stats)), _p(counts), _p(_f32c(dz)), _stream(dev)))


def cross_entropy_pair(z, ya, yb, lam, stats, weight=None, label_smoothing=0.0, counts=None, dz=None):
    """spk_op_cross_entropy_pair: the Mixup / CutMix criterion lam * CE(z, ya) + (1 - lam) * CE(z, yb) of
    CrossEntropyLoss(weight, label_smoothing).  Adds (n * loss, rows whose arg-max is the dominant label - ya when
    lam >= 0.5, else yb) to stats [2] float32 and per class (rows, correct rows) of the dominant label to counts [c, 2]
    int32 (None: no counters); writes dz [N,c] (the caller's buffer; None: no gradient).  yb None (or lam == 1): the bits
    of `cross_entropy_ex` on ya."""
    so = lib.load()
    dev = z.device
    n, c = z.shape
    for y in (ya, yb):
        assert y is None or (y.dtype == torch.int64 and y.is_contiguous() and y.is_cuda and y.numel() == n)
    assert weight is None or weight.numel() == c
    assert counts is None or (counts.dtype == torch.int32 and counts.is_contiguous() and counts.is_cuda
                              and counts.numel() == 2 * c)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_cross_entropy_pair(_p(_f32c(z)), _p(ya), _p(yb), float(lam), n, c, _p(_f32c(weight)),
                                               float(label_smoothing), _p(_f32c(stats)), _p(counts), _p(_f32c(dz)),
                                               _stream(dev)))


def cross_entropy_distill(z, ya, yb, lam, teacher, alpha, temperature, stats, weight=None, label_smoothing=0.0,
                          counts=None, kd_stats=None, dz=None):
    """spk_op_cross_entropy_distill: (1 - alpha) * L_hard + alpha * T^2 * KL(softmax(teacher / T) || softmax(z / T)),
    L_hard the criterion of `cross_entropy_pair` (yb None: of `cross_entropy_ex` on ya), T = temperature.  Adds (n * loss,
    correct rows) to stats [2] and the per-class counters to counts as there, and (n * KD, rows whose arg-max equals the
    teacher's) to kd_stats [2] float32 (None: not kept); writes dz [N,c] (None: no gradient).  teacher: float32 [N,c] on
    the device; None (or alpha == 0): the bits of `cross_entropy_pair`, kd_stats untouched."""
    so = lib.load()
    dev = z.device
    n, c = z.shape
    for y in (ya, yb):
        assert y is None or (y.dtype == torch.int64 and y.is_contiguous() and y.is_cuda and y.numel() == n)
    assert teacher is None or (teacher.is_cuda and tuple(teacher.shape) == (n, c))
    assert weight is None or weight.numel() == c
    assert counts is None or (counts.dtype == torch.int32 and counts.is_contiguous() and counts.is_cuda
                              and counts.numel() == 2 * c)
    assert kd_stats is None or kd_stats.numel() == 2
    with torch.cuda.device(dev):
        lib.check(so.spk_op_cross_entropy_distill(_p(_f32c(z)), _p(ya), _p(yb), float(lam), _p(_f32c(teacher)), float(alpha),
                                                  float(temperature), n, c, _p(_f32c(weight)), float(label_smoothing),
                                                  _p(_f32c(stats)), _p(counts), _p(_f32c(kd_stats)), _p(_f32c(dz)),
                                                  _stream(dev)))


def mix_batch(x, ca, cb, box, shift=1, out=None):
    """spk_mix_batch: x mixed with itself rolled by `shift` images along the batch.  x: a contiguous device batch, uint8
    [N,H,W,C] or float32 [N,C,H,W], C 1 or 3.  Inside box = (y1, x1, y2, x2) the result is ca * x[i] + cb * x[(i - shift)
    % N] (each product and the sum rounded to float32; uint8 rounds that to nearest-even and clamps), outside it x[i];
    (ca, cb) = (0, 1) copies the partner's pixels.  out: the caller's buffer of x's shape and dtype (it must not overlap
    x), else a new tensor.  Returns out; the work is enqueued on the current stream."""
    so = lib.load()
    dev = x.device
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4 and x.dtype in (torch.uint8, torch.float32), \
        "contiguous uint8 [N,H,W,C] or float32 [N,C,H,W] device batch expected"
    if x.dtype == torch.uint8:
        n, h, w, c = x.shape
        layout, dtype = lib.LAYOUT_NHWC, lib.DTYPE_U8
    else:
        n, c, h, w = x.shape
        layout, dtype = lib.LAYOUT_NCHW, lib.DTYPE_F32
    if out is None:
        out = torch.empty_like(x)
    assert out.is_cuda and out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
    y1, x1, y2, x2 = (int(v) for v in box)
    with torch.cuda.device(dev):
        lib.check(so.spk_mix_batch(_p(x), _p(out), n, h, w, c, layout, dtype, int(shift), float(ca), float(cb), y1, x1, y2,
                                   x2, _stream(dev)))
    return out


def tta_views(x, views, out=None):
    """spk_tta_views: the dihedral views of a batch, [k, *x.shape] view-major, out[j, i] = T_views[j](x[i]) bit for bit.
    x: a contiguous device batch, uint8 [N,H,W,C] or float32 [N,C,H,W], C 1 or 3.  views: 1 to 8 codes in 0..7 (bit
    value 4 transposes H and W first, 2 then reverses the rows, 1 the columns; see tta.py).  out: the caller's buffer of
    that shape and x's dtype (it must not overlap x), else a new tensor.  One launch, enqueued on the current stream."""
    so = lib.load()
    dev = x.device
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4 and x.dtype in (torch.uint8, torch.float32), \
        "contiguous uint8 [N,H,W,C] or float32 [N,C,H,W] device batch expected"
    if x.dtype == torch.uint8:
        n, h, w, c = x.shape
        layout, dtype = lib.LAYOUT_NHWC, lib.DTYPE_U8
    else:
        n, c, h, w = x.shape
        layout, dtype = lib.LAYOUT_NCHW, lib.DTYPE_F32
    codes = [int(v) for v in views]
    if out is None:
        out = torch.empty((len(codes),) + tuple(x.shape), dtype=x.dtype, device=dev)
    assert out.is_cuda and out.is_contiguous() and out.shape == (len(codes),) + tuple(x.shape) and out.dtype == x.dtype
    with torch.cuda.device(dev):
        lib.check(so.spk_tta_views(_p(x), _p(out), n, h, w, c, layout, dtype, (C.c_int32 * len(codes))(*codes), len(codes),
                                   _stream(dev)))
    return out


def tta_mean(p, out=None):
    """spk_tta_mean: p [k, ...] float32 (k in 1..8) -> the mean over the first dimension, ((p[0] + p[1]) + ...) / k in
    float32: adds in that order, then one IEEE division.  out: the caller's float32 buffer of shape p.shape[1:] (it must
    not overlap p), else a new tensor.  One launch, enqueued on the current stream."""
    so = lib.load()
    dev = p.device
    assert p.is_cuda and p.is_contiguous() and p.dtype == torch.float32 and p.dim() >= 2, \
        "contiguous float32 [k, ...] device tensor expected"
    if out is None:
        out = torch.empty(tuple(p.shape[1:]), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() * p.shape[0] == p.numel()
    with torch.cuda.device(dev):
        lib.check(so.spk_tta_mean(_p(p), _p(out), int(p.shape[0]), int(out.numel()), _stream(dev)))
    return out


def maxpool(x, k, stride, pad, want_idx=False):
    """MaxPool2d on x [N,H,W,C] bf16 / fp16 (spk_op_maxpool).  want_idx: the training kernel, which also returns the
    saved taps [N,Ho,Wo,C] uint8; else the eval kernel.  Returns (y, idx or None)."""
    so = lib.load()
    dev = x.device
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.full((n, ho, wo, c), float("nan"), dtype=x.dtype, device=dev)
    idx = torch.full((n, ho, wo, c), 255, dtype=torch.uint8, device=dev) if want_idx else None
    with torch.cuda.device(dev):
        lib.check(so.spk_op_maxpool(_p(_h16c(x)), _p(y), _p(idx), n, h, w, c, int(k), int(stride), int(pad),
                                    int(x.dtype == torch.float16), _stream(dev)))
    return y, idx


def maxpool_backward(gy, idx, in_hw, k, stride, pad, form=-1):
    """gx [N,H,W,C] bf16 from gy [N,Ho,Wo,C] bf16 and the saved taps (spk_op_maxpool_backward).  form: -1 production's
    kernel, 0 per-pixel, 1 pixel-pair."""
    so = lib.load()
    dev = gy.device
    n, _, _, c = gy.shape
    h, w = in_hw
    assert idx.dtype == torch.uint8 and idx.is_contiguous() and idx.shape == gy.shape
    gx = torch.full((n, h, w, c), float("nan"), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_maxpool_backward(_p(_bf16c(gy)), _p(idx), _p(gx), n, h, w, c, int(k), int(stride), int(pad),
                                             int(form), _stream(dev)))
    return gx


def gavgpool(x):
    """AdaptiveAvgPool2d(1) on x [N,HW,C] bf16 / fp16 -> float32 [N,C] (spk_op_gavgpool)."""
    so = lib.load()
    dev = x.device
    n, hw, c = x.shape
    y = torch.full((n, c), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_gavgpool(_p(_h16c(x)), _p(y), n, hw, c, int(x.dtype == torch.float16), _stream(dev)))
    return y


def gavgpool_backward(gy, hw):
    """gx [N,HW,C] bf16 = gy [N,C] / HW (spk_op_gavgpool_backward)."""
    so = lib.load()
    dev = gy.device
    n, c = gy.shape
    gx = torch.full((n, hw, c), float("nan"), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        lib.check(so.spk_op_gavgpool_backward(_p(_f32c(gy)), _p(gx), n, int(hw), c, _stream(dev)))
    return gx
