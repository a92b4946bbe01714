"""Build-time guard on the registers of the whole-bottleneck kernel (csrc/conv_bneck.hip), no GPU needed.

Phase 1 of the three-stage form loads its weight fragments with an instruction the compiler does not track
(`buffer_load_b128_untracked`, inline asm): its destination registers are valid only after the kernel's own
s_waitcnt.  If register pressure ever makes hipcc spill or copy them, the kernel silently reads a stale value - one
wrong image in a few hundred blocks (tests/test_gpu_bneck.py, test_blocks_that_share_and_inherit_cus).  So every
instantiation that contains that instruction must compile with no scratch and no spilled VGPRs."""

import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "syke-pic_amd" / "csrc"


def _hipcc():
    for c in (shutil.which("hipcc"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no hipcc: the library cannot be built here either")


def bneck_resources(tmp_path):
    """{(CM, HW, R, NW): {"vgprs", "scratch", "spills", "untracked"}} for every conv_bneck_kernel instantiation."""
    asm = tmp_path / "conv_bneck.s"
    out = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S",
                          "-Rpass-analysis=kernel-resource-usage", str(CSRC / "conv_bneck.hip"), "-o", str(asm)],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    name = re.compile(r"conv_bneck_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
    res, cur = {}, None
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            m = name.search(ln)
            cur = tuple(int(v) for v in m.groups()) if m else None
            if cur:
                res[cur] = {}
        elif cur:
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("spills", r"VGPRs Spill: (\d+)")):
                m = re.search(pat, ln)
                if m:
                    res[cur][key] = int(m.group(1))
    # which kernels hold the untracked load: inline asm is bracketed by ;;#ASMSTART / ;;#ASMEND in the assembly
    text = asm.read_text()
    for m in re.finditer(r"^(_Z\S*conv_bneck_kernel\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        key = tuple(int(v) for v in name.search(m.group(1)).groups())
        res[key]["untracked"] = bool(re.search(r";;#ASMSTART\s+buffer_load_dwordx4", m.group(2)))
    return res


def test_untracked_weight_loads_never_spill(tmp_path):
    res = bneck_resources(tmp_path)
    # the two forms the ResNet-50 inference step runs (stage 3 and stage 2, 14-row bands, 8 waves) and the 7-row forms
    assert {(256, 14, 14, 8), (128, 28, 14, 8), (256, 14, 7, 4), (128, 28, 7, 4)} <= set(res), sorted(res)
    for key, r in res.items():
        assert {"vgprs", "scratch", "spills", "untracked"} <= set(r), (key, r)
        assert r["vgprs"] <= 256, (key, r)
    untracked = {k: r for k, r in res.items() if r["untracked"]}
    assert untracked, "no instantiation uses buffer_load_b128_untracked: the guard checks nothing"
    for key, r in untracked.items():
        assert key[3] == 8, ("the untracked load belongs to the three-stage 8-wave form only", key)
        assert r["scratch"] == 0 and r["spills"] == 0, ("an instantiation with untracked loads spills", key, r)
