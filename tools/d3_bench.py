"""Times the 64 -> 64 3x3 conv of stage 1 (56 x 56) through spk_op_conv3x3_direct: the implicit GEMM (cfg -1) and every
configuration of the direct kernel (csrc/conv_d3.hip), in alternation over several rounds in one process.
usage: d3_bench.py [n ...]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "syke-pic_amd")]
import torch
from sykepic_hip import ops

ns = [int(v) for v in sys.argv[1:]] or [128, 256]
ROUNDS, ITERS = 5, 20
for n in ns:
    for with_res in (False, True):
        g = torch.Generator().manual_seed(1)
        x = torch.relu(torch.randn(n, 64, 56, 56, generator=g)).half().cuda()
        w = ((torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) * (6.0 / 576) ** 0.5).cuda()
        sc, sh = (0.5 + torch.rand(64, generator=g)).cuda(), (torch.rand(64, generator=g) - 0.5).cuda()
        res = torch.randn(n, 64, 56, 56, generator=g).half().cuda() if with_res else None
        gflop = 2.0 * n * 56 * 56 * 9 * 64 * 64 / 1e9
        mbytes = (2 + with_res) * n * 56 * 56 * 64 * 2 / 1e6
        cfgs = list(range(-1, ops.conv3x3_direct_num_configs()))
        times = {c: [] for c in cfgs}
        base = None
        for r in range(ROUNDS):
            for c in cfgs:
                y, ms = ops.conv3x3_direct(x, w, sc, sh, relu=True, cfg=c, res=res, iters=ITERS)
                times[c].append(ms * 1e3)
                if r == 0:
                    base = y if c < 0 else base
                    assert torch.equal(y, base), c
        print(f"n={n} 56x56 64->64 res={int(with_res)}: {gflop:.1f} GFLOP, {mbytes:.0f} MB compulsory", flush=True)
        for c in cfgs:
            t = sorted(times[c])
            med = t[len(t) // 2]
            print(f"  {'igemm' if c < 0 else 'd3 cfg %d' % c}: median {med:.1f} us (min {t[0]:.1f}, max {t[-1]:.1f}) = "
                  f"{gflop / med * 1e3:.0f} TFLOP/s, {mbytes / med * 1e3:.0f} GB/s", flush=True)
