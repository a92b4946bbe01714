"""The paired tags of the tuner table ("conv_p", "pw1x1_p", "pw2_p", "c3_p", "chain_p", "bneck_p", "d3_p":
csrc/tune_table.h) through the table's own parse / find / store path, without a GPU: spk_op_tune_table.  A paired line
has its isolated sibling's fields, is an entry of its own (neither tag answers for the other), follows the nearest-batch
rule, is appended to the cache file and read back by a fresh table, and is dropped on load when it is malformed - while
the isolated lines of the same file, the shipped seed's among them, parse as before.  The shipped paired winners
(tune_seed_gfx950_paired.txt) load whole, and a new default cache starts from the seed with them behind it.  The table is
process-wide, so the checks run in a child process with a cache file of its own."""

import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SEED = ROOT / "syke-pic_amd" / "sykepic_hip" / "tune_seed_gfx950.txt"
PSEED = ROOT / "syke-pic_amd" / "sykepic_hip" / "tune_seed_gfx950_paired.txt"

# tag -> (key fields, value fields, position of N in the key): kTuneSchemas
FIELDS = {"conv": (13, 2, 3), "pw1x1": (9, 1, 8), "pw2": (11, 1, 10), "c3": (6, 1, 5), "chain": (6, 1, 5),
          "bneck": (3, 1, 2), "d3": (4, 1, 3)}

CHILD = r"""
import ctypes, os, sys
sys.path[:0] = [%(root)r, %(pkg)r]
from sykepic_hip import lib
FIELDS = %(fields)r
cache = sys.argv[1]
os.environ["SPK_TUNE_CACHE"] = cache
so = lib.load()
os.environ["SPK_TUNE_CACHE"] = cache        # (load() may have chosen a default file)

def call(what, tag, key, vals):
    k = (ctypes.c_int * len(key))(*key)
    v = (ctypes.c_int * max(len(vals), 1))(*vals)
    found = ctypes.c_int(-1)
    rc = so.spk_op_tune_table(what, tag.encode(), k, len(key), v, len(vals), ctypes.byref(found))
    return rc, found.value, list(v)[:len(vals)]

def find(tag, key, nv):
    rc, found, v = call(0, tag, key, [0] * nv)
    assert rc == 0, so.spk_last_error()
    return v if found else None

def forget():
    assert so.spk_op_tune_table(2, None, None, 0, None, 0, None) == 0

forget()
# the shipped seed's lines first: what an older cache file looks like
seed = [ln for ln in open(%(seed)r).read().splitlines() if ln and not ln.startswith("#")]
old = [ln for ln in seed if not ln.split()[0].endswith("_p")]
assert len(old) >= 282
with open(cache, "w") as f:
    f.write("\n".join(old) + "\n")
forget()
for ln in old:
    tag, *ints = ln.split()
    ints = [int(x) for x in ints]
    if tag not in FIELDS:
        continue
    nk, nv, npos = FIELDS[tag]
    assert len(ints) == nk + nv, ln
    assert find(tag, ints[:nk], nv) == ints[nk:], ln             # isolated lines parse as before ...
    assert find(tag + "_p", ints[:nk], nv) is None, ln            # ... and answer no paired look-up

# one entry per paired tag: stored, found exactly and by the nearest batch, never under the sibling, appended
n_before = len(open(cache).read().splitlines())
mine = {}
for i, (tag, (nk, nv, npos)) in enumerate(sorted(FIELDS.items())):
    key = [7 + i] * nk                 # no network has such a problem: absent from the seed under both tags
    key[npos] = 96
    vals = [1] * nv
    assert find(tag + "_p", key, nv) is None and find(tag, key, nv) is None
    rc, _, _ = call(1, tag + "_p", key, vals)
    assert rc == 0
    mine[tag] = (key, vals)
    assert find(tag + "_p", key, nv) == vals
    assert find(tag, key, nv) is None, tag
    near, far, other = list(key), list(key), list(key)
    near[npos], far[npos] = 97, 96 * 2 + 1
    other[(npos + 1) %% nk] += 1
    assert find(tag + "_p", near, nv) == vals                    # a ragged twin half re-uses its neighbour's entry
    assert find(tag + "_p", far, nv) is None and find(tag + "_p", other, nv) is None
lines = open(cache).read().splitlines()
assert len(lines) == n_before + len(FIELDS)
for (tag, (key, vals)), ln in zip(sorted(mine.items()), lines[n_before:]):
    assert ln == " ".join([tag + "_p"] + [str(x) for x in key + vals]), ln

# a fresh table (what the next process sees) reads them back; malformed paired lines are dropped, their neighbours kept
with open(cache, "a") as f:
    f.write("c3_p 1 9 9 64 64 5\n")               # a field short
    f.write("c3_p 1 9 9 64 64 5 99\n")            # value out of range
    f.write("bneck_p 14 256 40 3\n")              # value out of range (forms 0..2)
    f.write("bneck_p 14 256 40 1 7\n")            # a field too many
    f.write("c3_q 1 9 9 64 64 5 3\n")             # no such tag
    f.write("c3_p1 9 9 64 64 5 3\n")              # no blank behind the tag
    f.write("bneck_p 28 128 40 1\n")              # fine
forget()
for tag, (key, vals) in mine.items():
    assert find(tag + "_p", key, len(vals)) == vals and find(tag, key, len(vals)) is None
assert find("c3_p", [1, 9, 9, 64, 64, 5], 1) is None
assert find("bneck_p", [14, 256, 40], 1) is None
assert find("bneck_p", [28, 128, 40], 1) == [1] and find("bneck", [28, 128, 40], 1) is None
tag, *ints = old[0].split()
if tag in FIELDS:
    nk, nv, _ = FIELDS[tag]
    assert find(tag, [int(x) for x in ints[:nk]], nv) == [int(x) for x in ints[nk:]]

# the shipped paired winners: every line an entry under its paired tag, none under the sibling's
pseed = [ln for ln in open(%(pseed)r).read().splitlines() if ln and not ln.startswith("#")]
assert pseed and all(ln.split()[0].endswith("_p") and ln.split()[0][:-2] in FIELDS for ln in pseed)
with open(cache, "w") as f:
    f.write("\n".join(pseed) + "\n")
forget()
for ln in pseed:
    tag, *ints = ln.split()
    ints = [int(x) for x in ints]
    nk, nv, _ = FIELDS[tag[:-2]]
    assert len(ints) == nk + nv, ln
    assert find(tag, ints[:nk], nv) == ints[nk:] and find(tag[:-2], ints[:nk], nv) is None, ln

# the hook refuses what is no tag or not its field counts
assert call(0, "c3_q", [1] * 6, [0])[0] != 0 and b"op_tune_table" in so.spk_last_error()
assert call(0, "c3_p", [1] * 5, [0])[0] != 0 and call(1, "conv_p", [1] * 13, [0])[0] != 0
print("paired tags ok")
"""


def test_paired_tags_parse_find_store(tmp_path):
    code = CHILD % dict(root=str(ROOT), pkg=str(ROOT / "syke-pic_amd"), fields=FIELDS, seed=str(SEED), pseed=str(PSEED))
    env = {k: v for k, v in os.environ.items() if k not in ("SPK_TUNE_LOG", "SPK_TUNE_PAIRED")}
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "tune.txt")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "paired tags ok" in r.stdout


def test_a_default_cache_starts_from_the_seed_and_the_paired_winners(tmp_path, monkeypatch):
    from sykepic_hip import lib
    assert lib.TUNE_SEED_PAIRED == PSEED and PSEED.is_file()
    monkeypatch.delenv("SPK_TUNE_SEED", raising=False)
    target = tmp_path / "tune.txt"
    assert lib.seed_tune_cache(str(target), extra=(lib.TUNE_SEED_PAIRED,)) is True
    assert target.read_text() == SEED.read_text() + PSEED.read_text()
    assert SEED.read_text().endswith("\n") and PSEED.read_text().endswith("\n")
    assert lib.seed_tune_cache(str(target), extra=(lib.TUNE_SEED_PAIRED,)) is False      # an existing cache is never touched
    for ln in PSEED.read_text().splitlines():
        assert ln.startswith("#") or (ln.split()[0].endswith("_p") and len(ln) < 250), ln
