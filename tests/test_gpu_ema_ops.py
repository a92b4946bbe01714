"""`ema_lerp_kernel` and `swap_f32_kernel` (csrc/train_kernels.hip) through `spk_op_ema_lerp` / `spk_op_swap_f32`, BIT
FOR BIT against the float64 oracle of tests/ema_util.py, which tests/test_host_ema.py proves equal to the correctly
rounded fused result on every element compared here.

Sizes 1 .. 262147: below one 16-byte chunk, around one wave / one block / four blocks of chunks, an odd count past
256 Ki (several rounds of the grid-stride loop on part of the grid).  Each buffer starts 0 to 3 floats behind a 16-byte
boundary - the same offset for both (16-byte reads of `p`, with a scalar head) and different ones (element reads of
`p`) - between guard bands that must come back untouched, as must `p`."""

import ctypes as C

import numpy as np
import pytest
import torch

import ema_util as U

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 262147]
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0), (2, 3), (3, 2), (0, 2), (1, 3)]     # (written, other), in floats
GUARD = 8
SENTINEL = np.float32(-1234.5)


def _so():
    from sykepic_hip import lib
    return lib.load()


def _placed(values, off):
    """(flat, view): a device buffer of GUARD + off sentinels (its base is 16-byte aligned), the values, GUARD more."""
    n = len(values)
    flat = torch.full((GUARD + off + n + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[GUARD + off:GUARD + off + n]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 * off
    return flat, view


def _guards_intact(flat, off, n):
    f = U.bits(flat.cpu().numpy())
    s = U.bits1(SENTINEL)
    return bool((f[:GUARD + off] == s).all()) and bool((f[GUARD + off + n:] == s).all())


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", SIZES)
def test_lerp_equals_the_oracle_bitwise(n):
    so = _so()
    e, p = U.inputs(n)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for w in U.WEIGHTS:
        want = U.bits(U.oracle(e, p, w))
        for eo, po in OFFSETS:
            ef, ev = _placed(e, eo)
            pf, pv = _placed(p, po)
            rc = so.spk_op_ema_lerp(_ptr(ev), _ptr(pv), n, w, stream)
            assert rc == 0, so.spk_last_error()
            got = U.bits(ev.cpu().numpy())
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (n, w, eo, po, bad[:5], got[bad[:5]], want[bad[:5]])
            assert _guards_intact(ef, eo, n) and _guards_intact(pf, po, n), (n, w, eo, po)
            assert np.array_equal(U.bits(pv.cpu().numpy()), U.bits(p)), (n, w, eo, po)
        # the planted cases, against their stated bits (the first len(PLANTED) elements, as many as fit)
        for i, (pe, pp, stated) in enumerate(U.PLANTED[:n]):
            if stated is not None:
                assert int(want[i]) == U.bits1(stated), (i, pe, pp)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bitwise_and_twice_restores(n):
    so = _so()
    a, b = U.inputs(n)               # (-0, denormals and 1e30 among them: a swap moves bits, whatever they are)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ao, bo in OFFSETS:
        af, av = _placed(a, ao)
        bf, bv = _placed(b, bo)
        assert so.spk_op_swap_f32(_ptr(av), _ptr(bv), n, stream) == 0, so.spk_last_error()
        assert np.array_equal(U.bits(av.cpu().numpy()), U.bits(b)), (n, ao, bo)
        assert np.array_equal(U.bits(bv.cpu().numpy()), U.bits(a)), (n, ao, bo)
        assert _guards_intact(af, ao, n) and _guards_intact(bf, bo, n), (n, ao, bo)
        assert so.spk_op_swap_f32(_ptr(av), _ptr(bv), n, stream) == 0, so.spk_last_error()
        assert np.array_equal(U.bits(av.cpu().numpy()), U.bits(a)) and np.array_equal(U.bits(bv.cpu().numpy()), U.bits(b))
        assert _guards_intact(af, ao, n) and _guards_intact(bf, bo, n), (n, ao, bo)
