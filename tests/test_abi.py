"""The C-ABI library loads (no GPU needed) and exports every symbol that
include/sykepic_hip.h declares; the ctypes table covers the same set."""

import ctypes
import re
from pathlib import Path

import pytest

from sykepic_hip import lib

ROOT = Path(__file__).resolve().parent.parent


def _declared():
    text = (ROOT / "include" / "sykepic_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(spk_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    names = _declared()
    assert len(names) >= 20
    assert lib.LIB_PATH.is_file(), "run __graft_entry__.build() first"
    so = ctypes.CDLL(str(lib.LIB_PATH))
    for n in names:
        assert hasattr(so, n), f"{n} declared in the header but not exported"
    assert sorted(lib.SYMBOLS) == names
    lib.load()


def test_error_reporting_without_gpu_or_bad_args():
    so = lib.load()
    assert b"gfx950" in so.spk_version()
    h = ctypes.c_void_p()
    rc = so.spk_model_create(None, 0, 3, 50, 0, ctypes.byref(h))
    assert rc != 0 and so.spk_last_error()
    # the head / loss / pooling hooks check their arguments before any HIP call: one rejected call each
    ARG, UNSUPPORTED = -1, -4      # SPK_ERR_ARG, SPK_ERR_UNSUPPORTED
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = [
        ("spk_op_linear", ARG, (None, p, None, p, 1, 4, 4, None)),
        ("spk_op_linear", ARG, (p, p, None, p, 0, 4, 4, None)),
        ("spk_op_linear_backward", ARG, (p, None, p, p, None, None, 1, 4, 4, -1, None)),      # dw without x
        ("spk_op_linear_backward", ARG, (p, p, p, None, None, None, 1, 4, 4, -1, None)),      # nothing to compute
        ("spk_op_linear_backward", ARG, (p, p, p, p, p, p, 1, 4, 4, 2, None)),                # form
        ("spk_op_softmax", ARG, (p, None, 1, 4, 1.3, None)),
        ("spk_op_softmax", ARG, (p, p, 1, 4, 0.0, None)),
        ("spk_op_cross_entropy", ARG, (p, p, 1, 4, None, None, None)),
        ("spk_op_cross_entropy", ARG, (p, p, 0, 4, p, None, None)),
        ("spk_op_maxpool", ARG, (p, p, None, 1, 4, 4, 12, 3, 2, 1, 0, None)),                 # c % 8
        ("spk_op_maxpool", ARG, (p, None, None, 1, 4, 4, 8, 3, 2, 1, 0, None)),
        ("spk_op_maxpool", ARG, (p, p, None, 1, 4, 4, 8, 3, 2, 1, 2, None)),                  # dtype
        ("spk_op_maxpool", UNSUPPORTED, (p, p, p, 1, 40, 40, 8, 16, 2, 1, 0, None)),          # k * k > 255
        ("spk_op_maxpool", UNSUPPORTED, (p, p, p, 1, 4, 4, 8, 3, 2, 1, 1, None)),             # saved taps in fp16
        ("spk_op_maxpool_backward", ARG, (p, None, p, 1, 4, 4, 8, 3, 2, 1, -1, None)),
        ("spk_op_maxpool_backward", ARG, (p, p, p, 1, 4, 4, 12, 3, 2, 1, -1, None)),          # c % 8
        ("spk_op_maxpool_backward", UNSUPPORTED, (p, p, p, 1, 4, 5, 8, 3, 2, 1, 1, None)),    # pair kernel, odd width
        ("spk_op_maxpool_backward", UNSUPPORTED, (p, p, p, 1, 4, 4, 8, 3, 1, 1, 1, None)),    # pair kernel, stride 1
        ("spk_op_gavgpool", ARG, (p, p, 0, 4, 8, 0, None)),
        ("spk_op_gavgpool", ARG, (p, p, 1, 4, 12, 0, None)),
        ("spk_op_gavgpool_backward", ARG, (None, p, 1, 4, 8, None)),
        ("spk_op_gavgpool_backward", ARG, (p, p, 1, 4, 12, None)),
        # the MBConv eval / eval stem hooks: (x, w, scale, bias, res, gate, y, n, h, w, cin, cout, act, split, stream)
        ("spk_op_conv1x1_padded", ARG, (None, p, p, p, None, None, p, 1, 2, 2, 8, 8, 0, 0, None)),
        ("spk_op_conv1x1_padded", ARG, (p, None, p, p, None, None, p, 1, 2, 2, 8, 8, 0, 0, None)),
        ("spk_op_conv1x1_padded", ARG, (p, p, p, p, None, None, None, 1, 2, 2, 8, 8, 0, 0, None)),
        ("spk_op_conv1x1_padded", ARG, (p, p, p, p, None, None, p, 1, 2, 2, 12, 8, 0, 0, None)),     # cin % 8
        ("spk_op_conv1x1_padded", ARG, (p, p, p, p, None, None, p, 1, 2, 2, 8, 12, 0, 0, None)),     # cout % 8
        ("spk_op_conv1x1_padded", ARG, (p, p, p, p, None, None, p, 0, 2, 2, 8, 8, 0, 0, None)),      # n < 1
        ("spk_op_conv1x1_padded", ARG, (p, p, p, p, None, None, p, 1, 2, 2, 8, 8, 4, 0, None)),      # act
        # (x, partial, chunks, w1, b1, w2, b2, hid, scale, y, n, hw, c, sq, gate_kind, stream)
        ("spk_op_se_eval", ARG, (None, None, 1, p, p, p, p, p, p, None, 1, 4, 8, 2, 0, None)),
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, None, p, None, 1, 4, 8, 2, 0, None)),
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, p, p, p, 1, 4, 8, 2, 0, None)),             # y without x
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, p, p, None, 1, 4, 12, 2, 0, None)),         # c % 8
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, p, p, None, 0, 4, 8, 2, 0, None)),          # n < 1
        ("spk_op_se_eval", ARG, (None, p, 0, p, p, p, p, p, p, None, 1, 4, 8, 2, 0, None)),          # chunks < 1
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, p, p, None, 1, 4, 8, 2, 2, None)),          # gate_kind
        ("spk_op_se_eval", ARG, (None, p, 1, p, p, p, p, p, p, None, 1, 4, 8, 2, 0, None)),          # hid not behind scale
        # (x, w, scale, bias, y, n, h, w, cout, act, stream)
        ("spk_op_stem3_eval", ARG, (None, p, p, p, p, 1, 4, 4, 8, 0, None)),
        ("spk_op_stem3_eval", ARG, (p, p, p, p, None, 1, 4, 4, 8, 0, None)),
        ("spk_op_stem3_eval", ARG, (p, p, p, p, p, 1, 4, 4, 12, 0, None)),                           # cout % 8
        ("spk_op_stem3_eval", ARG, (p, p, p, p, p, 0, 4, 4, 8, 0, None)),                            # n < 1
        ("spk_op_stem3_eval", ARG, (p, p, p, p, p, 1, 4, 4, 8, 7, None)),                            # act
        ("spk_op_stem3_eval", UNSUPPORTED, (p, p, p, p, p, 1, 4, 4, 264, 0, None)),                  # cout > 256
        # (x, w, scale, bias, y, pool_y, n, h, w, split, stream)
        ("spk_op_stem7_eval", ARG, (None, p, p, p, p, None, 1, 8, 8, 0, None)),
        ("spk_op_stem7_eval", ARG, (p, p, p, None, p, None, 1, 8, 8, 0, None)),
        ("spk_op_stem7_eval", ARG, (p, p, p, p, None, None, 1, 8, 8, 0, None)),                      # neither output
        ("spk_op_stem7_eval", ARG, (p, p, p, p, p, None, 0, 8, 8, 0, None)),                         # n < 1
        ("spk_op_mbconv_eval_geometry", ARG, (0, 1, 1, 12, 2, ctypes.cast(buf, ctypes.POINTER(ctypes.c_int)))),   # c % 8
        ("spk_op_mbconv_eval_geometry", ARG, (9, 1, 1, 8, 2, ctypes.cast(buf, ctypes.POINTER(ctypes.c_int)))),    # kind
        ("spk_op_mbconv_eval_geometry", ARG, (3, 7, 0, 64, 0, ctypes.cast(buf, ctypes.POINTER(ctypes.c_int)))),   # tile config
    ]
    for name, want, args in bad:
        rc = getattr(so, name)(*args)
        assert rc == want, f"{name}{args[-9:]}: rc {rc}, expected {want}"
        assert name[4:].encode() in so.spk_last_error(), (name, so.spk_last_error())


def test_struct_layouts_match_header():
    assert ctypes.sizeof(lib.LayerDesc) == 11 * 4 + 4 + 96 + 96
    assert ctypes.sizeof(lib.OptimDesc) == 4 + 12 + 12 + 4 + 4 + 4 + 16
    assert ctypes.sizeof(lib.LayerTime) == 96 + 4 + 4 + 8 + 8  # 4 B padding before the doubles


def test_host_code_under_address_and_ub_sanitizers():
    """`csrc/build_asan.sh`: every translation unit with -fsanitize=address,undefined on its host pass + csrc/
    asan_driver.hip, which walks handle creation and its error paths, the parameter table (with a deliberately short
    key buffer), spk_last_error and the tuner table: one parser for the seven tags of the tune-cache file (valid,
    out-of-range, truncated, garbage, comment and over-long lines), the nearest-batch rule, the SPK_TUNE_CACHE path
    rule, and the shipped seed (argv[1]) loaded and written back line for line through the function that appends.
    Without a GPU every HIP call fails and the error paths run; a sanitizer report aborts the driver (exit != 0)."""
    import os
    import subprocess
    csrc = ROOT / "syke-pic_amd" / "csrc"
    recipe = csrc / "build_asan.sh"
    if os.path.exists("/dev/kfd"):
        pytest.skip("an AMD GPU is present: the sanitizer pass runs on hosts without one (every HIP call fails there)")
    exe = csrc / "build" / "asan" / "asan_driver"
    srcs = list(csrc.glob("*.hip")) + list(csrc.glob("*.h"))
    if not exe.is_file() or any(f.stat().st_mtime > exe.stat().st_mtime for f in srcs):
        subprocess.run(["bash", str(recipe)], check=True, timeout=1500)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("SPK_TUNE_CACHE", None)
    seed = ROOT / "syke-pic_amd" / "sykepic_hip" / "tune_seed_gfx950.txt"
    r = subprocess.run([str(exe), str(seed)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "asan_driver: ok" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
