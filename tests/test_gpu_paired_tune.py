"""Paired tuning (csrc/tune_table.h): the half batches of a two-stream eval forward tune their kernels beside their
twin and keep the winners under "<tag>_p" entries of the tuner table.  Which candidate runs never shows in the output,
so the logits of ResNet-18 and ResNet-50 on 64 and 65 images of 64 x 64 (the smallest batch that takes two streams; the
odd one makes the halves two different problems) are the same bits with SPK_TUNE_PAIRED=1, with SPK_TUNE_PAIRED=0, with
SPK_AUTOTUNE=0 and in a second process started on the first one's cache.  The table is process-wide: every configuration
is a child process with a cache file of its own (ResNet-50 in the calibrated mode, which reaches the chained and the
dual-source 1x1 kernels; at 64 x 64 the maps are 16 x 16 ... 2 x 2, so the whole-bottleneck kernel - 28 x 28 and 14 x 14
only - is not reached here: its paired chooser is what tools/paired_tune_report.py records on the benchmark's shape)."""

import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

# tag -> key + value fields of its line (kTuneSchemas); a paired line has its sibling's
FIELDS = {"conv": 15, "pw1x1": 10, "pw2": 12, "c3": 7, "chain": 7, "bneck": 4, "wgrad": 9, "d3": 5}
N_POS = {"conv": 3, "pw1x1": 8, "pw2": 10, "c3": 5, "chain": 5, "bneck": 2, "d3": 3}

CODE = (
    "import sys, numpy as np, torch\n"
    f"sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'syke-pic_amd')!r}]\n"
    "from sykepic_hip import arch, synth\n"
    "from sykepic_hip.net import HipNet\n"
    "network, n, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]\n"
    "g = arch.build_graph(network, 50)\n"
    "sd = synth.synth_state_dict(arch.param_specs(g), seed=2)\n"
    "net = HipNet(network, 50, weights=None)\n"
    "net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}); net.eval()\n"
    "if network == 'resnet50':\n"
    "    net.calibrate(torch.from_numpy(synth.synth_images(8, 3, 64, 64, seed=9000)).cuda())\n"
    "    net.set_precision('calibrated')\n"
    "x = torch.from_numpy(synth.synth_images(n, 3, 64, 64, seed=5)).cuda()\n"
    "z1 = net.forward(x).cpu().numpy()\n"      # the first forward of the shape: both halves on one stream, tuners at work
    "z2 = net.forward(x).cpu().numpy()\n"      # the two-stream forward on what they chose
    "assert np.isfinite(z1).all() and np.array_equal(z1, z2)\n"
    "np.save(out, z1)\n")


def _run(tmp_path, name, network, n, cache, **env):
    """One child process: (logits, stderr, lines of the cache file afterwards)."""
    out = tmp_path / f"{name}.npy"
    full = {k: v for k, v in os.environ.items() if k not in ("SPK_TUNE_PAIRED", "SPK_AUTOTUNE", "SPK_EVAL_STREAMS")}
    full.update(SPK_TUNE_CACHE=str(cache), SPK_TUNE_SEED="0", SPK_TUNE_LOG="1", **env)
    r = subprocess.run([sys.executable, "-c", CODE, network, str(n), str(out)], env=full, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = Path(cache).read_text().splitlines() if Path(cache).is_file() else []
    return np.load(out), r.stderr, lines


_paired = {}


@pytest.fixture
def paired(request, tmp_path_factory):
    """The SPK_TUNE_PAIRED=1 run of (network, n) from an empty cache, once per module: the reference of every test."""
    key = (request.getfixturevalue("network"), request.getfixturevalue("n"))
    if key not in _paired:
        d = tmp_path_factory.mktemp(f"paired_{key[0]}_{key[1]}")
        z, err, lines = _run(d, "paired", key[0], key[1], d / "tune.txt", SPK_TUNE_PAIRED="1")
        z.setflags(write=False)
        _paired[key] = (z, err, tuple(lines), d / "tune.txt")
    return _paired[key]


def _tags(lines):
    return {ln.split()[0] for ln in lines}


CASES = [("resnet18", 64), ("resnet18", 65), ("resnet50", 64), ("resnet50", 65)]


@pytest.mark.parametrize("config", ["unpaired", "no_autotune", "second_process"])
@pytest.mark.parametrize("network,n", CASES)
def test_logits_do_not_depend_on_how_the_kernels_were_tuned(tmp_path, paired, network, n, config):
    z, _, lines, cache = paired
    if config == "unpaired":
        z2, _, lines2 = _run(tmp_path, config, network, n, tmp_path / "tune.txt", SPK_TUNE_PAIRED="0")
        assert lines2 and not any(t.endswith("_p") for t in _tags(lines2)), _tags(lines2)
    elif config == "no_autotune":
        z2, _, lines2 = _run(tmp_path, config, network, n, tmp_path / "tune.txt", SPK_AUTOTUNE="0")
        assert not lines2, lines2[:5]                         # nothing timed: nothing to remember
    else:
        mine = tmp_path / "tune.txt"
        mine.write_text("\n".join(lines) + "\n")
        z2, err2, lines2 = _run(tmp_path, config, network, n, mine, SPK_TUNE_PAIRED="1")
        assert "[spk tune" not in err2, err2[-2000:]          # nothing tuned again,
        assert tuple(lines2) == lines                         # nothing appended
    print(network, n, config, "sha", hashlib.sha256(z.tobytes()).hexdigest()[:16], hashlib.sha256(z2.tobytes()).hexdigest()[:16])
    assert z.shape == (n, 50) and np.array_equal(z, z2)


@pytest.mark.parametrize("network,n", CASES)
def test_paired_run_writes_paired_lines_beside_parsable_isolated_ones(paired, network, n):
    _, err, lines, _ = paired
    tags = _tags(lines)
    print(network, n, sorted(tags))
    halves = {n // 2, n - n // 2}
    for ln in lines:
        tag, *ints = ln.split()
        base = tag[:-2] if tag.endswith("_p") else tag
        assert base in FIELDS and len(ints) == FIELDS[base], ln       # every line, isolated or paired: its tag's fields
        [int(v) for v in ints]
        if tag.endswith("_p"):
            assert int(ints[N_POS[base]]) in halves, ln               # paired entries: half-batch problems only
    # (ResNet-18's 64 -> 64 3x3 convs read the trunk and keep hi + lo weights: conv_c3.hip, not the direct kernel)
    want = {"conv_p", "pw1x1_p", "c3_p"} | ({"pw2_p", "chain_p", "d3_p"} if network == "resnet50" else set())
    assert want <= tags, (want - tags, tags)
    if network == "resnet50":                                         # (the calibration forward of 8 images: one stream)
        assert any(not t.endswith("_p") for t in tags), tags
    assert "[spk tune paired] conv_p " in err


def test_one_stream_and_a_small_batch_write_no_paired_line(tmp_path):
    _, _, one = _run(tmp_path, "one_stream", "resnet50", 64, tmp_path / "one.txt", SPK_EVAL_STREAMS="1")
    _, _, small = _run(tmp_path, "small", "resnet50", 32, tmp_path / "small.txt")
    for lines in (one, small):
        assert lines and not any(t.endswith("_p") for t in _tags(lines)), _tags(lines)


@pytest.mark.parametrize("network,n", [("resnet50", 64)])
def test_a_missing_paired_entry_is_tuned_not_answered_by_its_isolated_sibling(tmp_path, paired, network, n):
    """A cache with the isolated entries of the half-batch problems (written by an SPK_TUNE_PAIRED=0 run) and no paired
    one: the paired run tunes every one of them - its log and the lines it appends say so."""
    z, _, lines, _ = paired
    cache = tmp_path / "tune.txt"
    _, _, iso = _run(tmp_path, "isolated", network, n, cache, SPK_TUNE_PAIRED="0")
    half = [ln for ln in iso if ln.split()[0] in N_POS and int(ln.split()[1 + N_POS[ln.split()[0]]]) == n // 2]
    assert {"conv", "pw1x1", "d3"} <= _tags(half), _tags(half)      # the isolated siblings are there
    z2, err, after = _run(tmp_path, "paired_on_isolated", network, n, cache, SPK_TUNE_PAIRED="1")
    assert tuple(after[:len(iso)]) == tuple(iso)
    added = after[len(iso):]
    assert added and all(ln.split()[0].endswith("_p") for ln in added), added[:5]
    assert _tags(added) == {t for t in _tags(lines) if t.endswith("_p")}
    assert err.count("[spk tune paired] ") == len(added)
    assert np.array_equal(z, z2)
