"""Test-time augmentation: what the two kernels cost beside the forwards they feed (profiles/tta.txt).

Device events around back-to-back launches of `spk_tta_views` (both batch kinds, `flip` and `dihedral`), of k
`hipMemcpyAsync` device-to-device copies of the same batch (the least any k-view kernel could move), of `spk_tta_mean`,
and of the k eval forwards of a calibrated ResNet-18 at batch 512, 180 x 180; then `sykepic prob` on one synthetic
20 k-ROI sample with `--tta none / flip / dihedral`.  usage: tta_profile.py [OUT.txt] [n_roi]"""
import ctypes
import shutil
import sys
import tempfile
import time
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "syke-pic_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sykepic_hip import arch, ops, prob, synth, tta  # noqa: E402
from sykepic_hip.net import HipNet  # noqa: E402

N, HW, CLASSES = 512, 180, 50
ROUNDS, REPS, WARM = 5, 50, 10
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=REPS, rounds=ROUNDS, warm=WARM):
    """ms per call: device events around `reps` back-to-back calls, `rounds` times."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def fmt(ts, unit="us"):
    k = 1000.0 if unit == "us" else 1.0
    d = 1 if unit == "us" else 3
    return f"{np.median(ts) * k:.{d}f} {unit} ({', '.join(f'{t * k:.{d}f}' for t in ts)})"


hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipMemcpyAsync.restype = ctypes.c_int


def copies(x, out):
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = x.numel() * x.element_size()
    for j in range(out.shape[0]):
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(out[j].data_ptr()), ctypes.c_void_p(x.data_ptr()), nbytes, 3, stream)
        assert rc == 0, rc


say(f"Test-time augmentation kernels, one MI355X, one process.  Batch {N} x {HW} x {HW} x 3.  Device events around {REPS}")
say(f"back-to-back launches, {ROUNDS} rounds (median first, then the rounds), {WARM} warm-up launches.  The same buffers are")
say("used by every launch: the 50 MB uint8 batch and part of the `flip` output fit the 256 MiB Infinity Cache, so the GB/s")
say("and the kernel / copies ratios of the uint8 rows are not HBM rates; the in-situ lines below (`probabilities_tta` minus")
say("the k forwards alone) are what a `prob` run pays.")
say()
g = torch.Generator().manual_seed(0)
u8 = torch.randint(0, 256, (N, HW, HW, 3), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
f32 = (u8.permute(0, 3, 1, 2).float() / 255.0).contiguous()
view_ms = {}
for name, x in (("uint8 NHWC", u8), ("float32 NCHW", f32)):
    for mode in ("flip", "dihedral"):
        views = tta.views_of(mode)
        out = torch.empty((len(views),) + tuple(x.shape), dtype=x.dtype, device="cuda")
        tv = timed(lambda: ops.tta_views(x, views, out=out))
        tc = timed(lambda: copies(x, out))
        moved = x.numel() * x.element_size() * (1 + len(views))
        view_ms[(name, mode)] = float(np.median(tv))
        say(f"{name:12s} {mode:8s} k={len(views)}: view kernel {fmt(tv)}, {moved / np.median(tv) / 1e6:.0f} GB/s over "
            f"{moved / 1e6:.0f} MB")
        say(f"{'':12s} {'':8s}      {len(views)} hipMemcpyAsync device-to-device copies {fmt(tc)}; kernel / copies = "
            f"{np.median(tv) / np.median(tc):.2f}")
        del out
del f32
mean_ms = {}
for mode in ("flip", "dihedral"):
    k = len(tta.views_of(mode))
    p = torch.softmax(torch.randn((k, N, CLASSES), generator=g), dim=2).cuda()
    out = torch.empty((N, CLASSES), dtype=torch.float32, device="cuda")
    tm = timed(lambda: ops.tta_mean(p, out=out))
    mean_ms[mode] = float(np.median(tm))
    say(f"mean kernel  {mode:8s} k={k}: {fmt(tm)} for [{k}, {N}, {CLASSES}] float32")
say()

network = "resnet18"
sd = synth.synth_state_dict(arch.param_specs(arch.build_graph(network, CLASSES)), seed=2)
net = HipNet(network, CLASSES, weights=None)
net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
net.eval()
net.calibrate(u8[:256])
net.set_precision("calibrated")
say(f"{network}, calibrated single-pass mode (what `prob` runs), batch {N}, {HW} x {HW}, uint8 NHWC, ms per call, 5 rounds of 10:")
t1 = timed(lambda: net.probabilities(u8), reps=10, warm=5)
say(f"  one forward                      : {fmt(t1, 'ms')}  = {N / np.median(t1) * 1e3:.0f} img/s")
for mode in ("flip", "dihedral"):
    views = tta.views_of(mode)
    k = len(views)
    xv = ops.tta_views(u8, views)
    p = torch.empty((k, N, CLASSES), dtype=torch.float32, device="cuda")

    def forwards():
        for j in range(k):
            net.forward(xv[j], softmax_base=1.3, out=p[j])
    tf = timed(forwards, reps=10, warm=3)
    tt = timed(lambda: net.probabilities_tta(u8, views), reps=10, warm=3)
    both = view_ms[("uint8 NHWC", mode)] + mean_ms[mode]
    share = both / float(np.median(tf))
    say(f"  {mode:8s} {k} forwards           : {fmt(tf, 'ms')}")
    say(f"  {mode:8s} probabilities_tta     : {fmt(tt, 'ms')}")
    say(f"  {mode:8s} view + mean kernels   : {both * 1000:.1f} us = {100 * share:.2f} % of the {k} forwards; bound 5 %: "
        f"{'met' if share < 0.05 else 'NOT met'}")
    extra = float(np.median(tt)) - float(np.median(tf))
    say(f"  {mode:8s} in situ               : probabilities_tta - forwards = {extra * 1000:.0f} us = "
        f"{100 * extra / float(np.median(tf)):.2f} % of the {k} forwards (the two kernels, the allocation of their buffers "
        f"and the launches' host time); bound 5 %: {'met' if extra / float(np.median(tf)) < 0.05 else 'NOT met'}")
    del xv, p
del net, u8
torch.cuda.empty_cache()
say()

n_roi = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
tmp = Path(tempfile.mkdtemp())
rng = np.random.RandomState(0)
adc, blobs, off = [], [], 0
for i in range(n_roi):
    h, w = int(rng.randint(20, 120)), int(rng.randint(30, 300))
    cols = ["0"] * 24
    cols[15], cols[16], cols[17] = str(w), str(h), str(off)
    adc.append(",".join(cols))
    blobs.append(rng.randint(0, 256, h * w).astype(np.uint8))
    off += h * w
raw = tmp / "raw"
raw.mkdir()
(raw / "D20200101T000000_IFCB114.adc").write_text("\n".join(adc) + "\n")
np.concatenate(blobs).tofile(raw / "D20200101T000000_IFCB114.roi")
model = tmp / "model"
model.mkdir()
torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, model / "best_state.pth")
(model / "class_names.txt").write_text("\n".join(f"class_{i}" for i in range(CLASSES)))
(model / "config.ini").write_text((ROOT / "tests/golden/ref_data/config.ini").read_text())
Args = namedtuple("Args", "raw samples image_dir images model out batch_size num_workers force tta")
say(f"`sykepic prob` on one synthetic sample of {n_roi} ROIs ({off / 1e6:.0f} MB .roi), {network} 180 x 180, batch 512, one call per")
say("mode after a first call that loads, tunes and calibrates (act_means.pth is written by it); wall clock of the call,")
say("model load included, three calls per mode, alternating:")
prob.call(Args(str(raw), None, None, None, str(model), tmp / "warm", 512, 2, True, "none"))
prob.call(Args(str(raw), None, None, None, str(model), tmp / "warm", 512, 2, True, "dihedral"))
rates = {m: [] for m in ("none", "flip", "dihedral")}
for r in range(3):
    for mode in rates:
        t0 = time.perf_counter()
        prob.call(Args(str(raw), None, None, None, str(model), tmp / f"out_{mode}", 512, 2, True, mode))
        torch.cuda.synchronize()
        rates[mode].append(n_roi / (time.perf_counter() - t0))
for mode, rs in rates.items():
    say(f"  --tta {mode:8s}: {np.median(rs):.0f} ROI/s ({', '.join(f'{v:.0f}' for v in rs)})")
shutil.rmtree(tmp)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
