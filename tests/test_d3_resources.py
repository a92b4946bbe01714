"""Build-time guard on the registers of the direct 64 -> 64 3x3 kernel (csrc/conv_d3.hip), no GPU needed.

Each configuration is meant for two blocks per CU (its 74 KB weight panel fits the LDS twice) or, for the 256-pixel
tile of eight waves (configuration 3), one: 4-wave blocks then have two waves per SIMD and 256 VGPRs each, 8-wave blocks
at two per CU four waves per SIMD and 128.  A spilled register would put scratch traffic into a loop whose point is that nothing but the activation
loads touches memory.  The table this test parses is recorded in profiles/r07_d3_resources.txt."""

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


def d3_resources(tmp_path):
    """{(MT, WAVES, PA, WPE, HAS_RES): {"vgprs", "scratch", "spills", "sgpr_spills"}} per conv_d3_kernel instantiation."""
    out = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S",
                          "-Rpass-analysis=kernel-resource-usage", str(CSRC / "conv_d3.hip"), "-o", str(tmp_path / "conv_d3.s")],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    name = re.compile(r"conv_d3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
    res, cur = {}, None
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            m = name.search(ln)
            cur = tuple(int(v) for v in m.groups()) if m else None
            if cur:
                res[cur] = {}
        elif cur:
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("spills", r"VGPRs Spill: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)")):
                m = re.search(pat, ln)
                if m:
                    res[cur][key] = int(m.group(1))
    return res


def test_no_instantiation_spills_and_each_fits_its_occupancy(tmp_path):
    res = d3_resources(tmp_path)
    assert len(res) >= 8 and len(res) % 2 == 0, sorted(res)        # every configuration with and without a shortcut
    for key, r in sorted(res.items()):
        print(key, r)
        assert {"vgprs", "scratch", "spills", "sgpr_spills"} <= set(r), (key, r)
        assert r["scratch"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, (key, r)
        wpe = key[3]                                               # waves per SIMD the configuration is launched for
        assert r["vgprs"] <= 512 // wpe, (key, r)
    assert {k[:4] for k in res if k[4]} == {k[:4] for k in res if not k[4]}
