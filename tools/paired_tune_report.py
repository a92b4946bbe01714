"""Paired tuning (csrc/tune_table.h), the evidence behind profiles/paired_tune.txt.

  paired_tune_report.py first [network=resnet50] [batch=256]
      One process, empty or warm cache as SPK_TUNE_CACHE says: the wall time of the first forward of the shape (the one
      that tunes) and the median of ten later ones.  With SPK_TUNE_LOG=2 the tuners' candidate lines go to stderr; the
      line "#### timed batch" separates the calibration forward (32 images, one stream, isolated entries) from them.
  paired_tune_report.py table isolated.log paired.log
      Two such stderr logs of the same shape, SPK_TUNE_PAIRED=0 and =1, both from an empty cache: every problem whose
      paired winner is not its isolated winner, with both candidates' times alone and as pairs (us per launch / pair).
"""
import collections
import os
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "syke-pic_amd")]


def first(network="resnet50", batch=256):
    import numpy as np
    import torch
    from sykepic_hip import arch, synth
    from sykepic_hip.net import HipNet
    batch = int(batch)
    g = arch.build_graph(network, 50)
    sd = synth.synth_state_dict(arch.param_specs(g), seed=2)
    net = HipNet(network, 50, weights=None)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net.eval()
    net.calibrate(torch.from_numpy(synth.synth_images(32, 3, 224, 224, seed=9000)).cuda())
    net.set_precision("calibrated")
    x = torch.from_numpy(synth.synth_images(batch, 3, 224, 224, seed=5)).cuda()
    torch.cuda.synchronize()
    os.write(2, b"#### timed batch\n")
    ts = []
    for _ in range(12):
        t0 = time.perf_counter()
        net.probabilities(x)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"{network} batch {batch} SPK_TUNE_PAIRED={os.environ.get('SPK_TUNE_PAIRED', '1')}: first forward {ts[0]:.1f} ms, "
          f"second {ts[1]:.2f} ms, median of the last ten {statistics.median(ts[2:]):.3f} ms")


# candidate line -> (family, candidate id, us); final line -> (family, problem)
CAND = [
    ("conv", re.compile(r"\[spk cand\] (.*): cfg (\d+) dma (\d+) ([\d.]+) us"), lambda m: f"cfg {m[2]} dma {m[3]}", 4),
    ("1x1", re.compile(r"\[spk pw cand\] (.*): (igemm|pw) (-?\d+) ([\d.]+) us"), lambda m: f"{m[2]} {m[3]}", 4),
    ("1x1 dual", re.compile(r"\[spk pw2 cand\] (.*): pw (\d+) ([\d.]+) us"), lambda m: f"pw {m[2]}", 3),
    ("d3", re.compile(r"\[spk d3 cand\] (.*): (igemm|d3) (-?\d+) ([\d.]+) us"), lambda m: f"{m[2]} {m[3]}", 4),
    ("3x3", re.compile(r"\[spk c3 cand\] (.*): cfg (\d+) ([\d.]+) us"), lambda m: f"cfg {m[2]}", 3),
]
FINAL = [
    ("conv", re.compile(r"\[spk tune\] (mode .*): cfg (\d+) dma (\d+) \(")),
    ("1x1", re.compile(r"\[spk tune 1x1\] (.*): (?:igemm|pw) -?\d+ \(")),
    ("1x1 dual", re.compile(r"\[spk tune 1x1 dual\] (.*): pw \d+ \(")),
    ("d3", re.compile(r"\[spk tune d3\] (.*): (?:igemm|d3) -?\d+ \(")),
    ("3x3", re.compile(r"\[spk tune 3x3\] (.*): cfg -?\d+ \(")),
]
WHOLE = [   # the choosers that log every form in their one line
    ("chain", re.compile(r"\[spk tune chain\] (.*): two kernels ([\d.]+) us, chained ([\d.]+) us"), ("two kernels", "chained")),
    ("bottleneck", re.compile(r"\[spk tune bottleneck\] N(\d+)(?:\+\d+)? (.*?),? (?:pairs: )?three kernels ([\d.]+) us, "
                              r"(?:one \(14-row blocks\) ([\d.]+) us, )?one \(7-row blocks\) ([\d.]+) us"), None),
]


def problems(path):
    """{(family, problem): {candidate: us}} of the part of the log behind the marker."""
    text = Path(path).read_text(errors="replace")
    text = text.split("#### timed batch", 1)[-1]
    pending = collections.defaultdict(dict)
    out = {}
    for ln in text.splitlines():
        for fam, rx, name, us in CAND:
            m = rx.search(ln)
            if m:
                pending[fam][name(m)] = float(m[us])
        for fam, rx in FINAL:
            m = rx.search(ln)
            if m:
                out[(fam, m[1])] = pending.pop(fam, {})
        m = WHOLE[0][1].search(ln)
        if m:
            out[("chain", m[1])] = {"two kernels": float(m[2]), "chained": float(m[3])}
        m = WHOLE[1][1].search(ln)
        if m:
            forms = {"three kernels": float(m[3]), "7-row blocks": float(m[5])}
            if m[4]:
                forms["14-row blocks"] = float(m[4])
            out[("bottleneck", f"N{m[1]} {m[2]}")] = forms
    return out


def table(iso_log, pair_log):
    iso, pair = problems(iso_log), problems(pair_log)
    print(f"{len(iso)} problems tuned alone, {len(pair)} as pairs, {len(set(iso) & set(pair))} in both")
    print("us: alone / as a pair.  The 1x1 and d3 choosers keep the implicit GEMM unless the other kernel wins by 8 %.")
    n = 0
    for key in sorted(set(iso) & set(pair)):
        a, p = iso[key], pair[key]
        if not a or not p:
            continue
        wa, wp = min(a, key=a.get), min(p, key=p.get)
        if wa == wp:
            continue
        n += 1
        f = lambda d, k: f"{d[k]:7.1f}" if k in d else "      -"   # noqa: E731
        print(f"{key[0]:10s} {key[1]}")
        print(f"    fastest alone   {wa:16s} alone {f(a, wa)}   pair {f(p, wa)}")
        print(f"    fastest in pair {wp:16s} alone {f(a, wp)}   pair {f(p, wp)}")
    print(f"{n} problems whose fastest candidate differs")
    for key in sorted(k for k in pair if k[0] == "bottleneck"):
        print("bottleneck", key[1], "pairs:", ", ".join(f"{k} {v:.1f} us" for k, v in pair[key].items()))


if __name__ == "__main__":
    {"first": first, "table": table}[sys.argv[1]](*sys.argv[2:])
