"""The cases of tests/test_gpu_mbconv_train_ops.py reach every launch-geometry branch of csrc/train_effnet.hip, and the
layers of the benchmark's EfficientNet training line (B0 and B4, batch 128, 224 x 224) land on branches those cases ran.

No GPU: the case lists are fed through `spk_op_mbconv_geometry`, which reports what the launchers' own helpers choose
(`walk_rows`, `walk_ctiles`, the channel tile of `RowWalk`, `spk_se_chunks`, `dw_wgrad_blocks`, `se_tile_rows`, the
depthwise dispatch, the NQ of `se_bwd1_kernel` and the SJ of `se_wgrad_kernel`)."""

import test_gpu_mbconv_train_ops as T
from sykepic_hip import arch, ops

WALK, DWW, POOL, SEG, FORM = 0, 1, 2, 3, 4
LDS, PX, GATHER = 0, 1, 2


def _flags(g):
    """(more than one channel tile, last tile narrower than the others, threads without a row)"""
    return (g[2] > 1, g[6] != g[3] // 8, g[5] > 0)


def _out(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _tested():
    t = {"walk_rows": set(), "walk_flags": set(), "dww_rows": set(), "dww_flags": set(), "chunks": set(),
         "pool_flags": set(), "ragged_chunk": set(), "nq": set(), "sj": set(), "gate_tiles": set(), "fwd": set(),
         "dgrad": set()}
    for (n, hw, C, cl) in T.BNA_SMALL_CASES + T.BNA_BIG_CASES:
        g = ops.mbconv_geometry(WALK, n * hw, C)
        t["walk_rows"].add(g[0])
        t["walk_flags"].add(_flags(g))
        t["rowscale_straddles"] = t.get("rowscale_straddles", False) or g[0] % hw != 0
    for (n, h, w, C, cl, k, s, pad) in T.DW_CASES + T.DW_BIG_CASES:
        ho, wo = _out(h, w, k, s, pad)
        g = ops.mbconv_geometry(DWW, n * ho * ((wo + 3) // 4), C)
        t["dww_rows"].add(g[0])
        t["dww_flags"].add(_flags(g))
    for (n, h, w, C, cl, k, s, pad) in T.DW_CASES:      # each runs dx with accumulate 0 and 1
        for acc in (0, 1):
            f = ops.mbconv_geometry(FORM, k, s, pad, acc)
            t["fwd"].add((k, s, f[0]))
            t["dgrad"].add((k, s, f[1], acc))
    for (n, hw, C, cl) in T.POOL_CASES + T.BNA_SMALL_CASES + T.BNA_BIG_CASES:
        g = ops.mbconv_geometry(POOL, c=C, hw=hw)
        t["chunks"].add(g[1])
        t["pool_flags"].add(_flags(g))
        if hw % g[1]:
            t["ragged_chunk"].add(g[1])
    for (n, hw, C, cl, S) in T.SE_CASES:
        g = ops.mbconv_geometry(POOL, c=C, hw=hw)
        t["chunks"].add(g[1])
        q = ops.mbconv_geometry(SEG, m=cl, s=S)
        t["nq"].add(q[2])
        t["gate_tiles"].add(min(q[1], 2))
    for (n, C, cl, S) in T.SE_WGRAD_CASES:
        t["sj"].add(ops.mbconv_geometry(SEG, m=cl, s=S)[3])
    return t


def test_cases_reach_every_geometry_branch():
    t = _tested()
    assert {64, 128, 1024} <= t["walk_rows"] and {64, 128, 1024} <= t["dww_rows"]
    assert t["chunks"] == {1, 4, 16} and {4, 16} <= t["ragged_chunk"]
    for key in ("walk_flags", "dww_flags", "pool_flags"):
        multi = {f for f in t[key] if f[0]}
        assert multi and any(f[1] for f in multi), f"{key}: no multi-tile / uneven-tile split in {t[key]}"
        assert any(f[2] for f in t[key]) and any(not f[2] for f in t[key]), f"{key}: idle threads"
    assert t["rowscale_straddles"]
    # per (k, stride): the four (form, accumulate) pairs a data gradient can take
    for k in (3, 5):
        assert {(k, 1, LDS, 0), (k, 1, PX, 1), (k, 1, GATHER, 0), (k, 1, GATHER, 1)} <= t["dgrad"]
        assert {(k, 2, PX, 0), (k, 2, PX, 1), (k, 2, GATHER, 0), (k, 2, GATHER, 1)} <= t["dgrad"]
        for s in (1, 2):
            assert {(k, s, LDS), (k, s, GATHER)} <= t["fwd"]
    assert t["nq"] == {3, 4}
    assert t["sj"] == {12, 13, 14, 15, 16}
    assert t["gate_tiles"] == {1, 2}     # one tile of W2 rows, and more than one
    for n in (1, 5, 33):
        assert any(c[0] == n for c in T.SE_WGRAD_CASES) and any(c[0] == n for c in T.SE_CASES)


def test_stem_cases_take_the_register_tile_kernel():
    """spk_launch_stem3_wgrad: cout % 4 == 0 and 9 cout / 4 <= 256 is the register-tile kernel; every stem of
    arch.build_graph and every case satisfies it (the other kernel is listed as unreachable in the GPU module)."""
    couts = {c[4] for c in T.STEM_CASES}
    for net in ("efficientnet_b0", "efficientnet_b4", "efficientnet_b7", "mobilenet_v3_large", "mobilenet_v3_small"):
        couts.add(arch.build_graph(net, 10).ops[0].cout)
    assert all(c % 4 == 0 and 9 * (c // 4) <= 256 for c in couts), couts


def _pad64(c):
    return (c + 63) // 64 * 64


def test_benchmark_shapes_land_on_tested_branches():
    t = _tested()
    n = 128
    for net in ("efficientnet_b0", "efficientnet_b4"):
        dims = {0: (224, 224)}
        for op in arch.build_graph(net, 50).ops:
            ih, iw = dims.get(op.src, (1, 1))
            if op.kind in (arch.OP_CONV, arch.OP_DWCONV):
                oh, ow = _out(ih, iw, op.k, op.stride, op.pad)
                dims[op.dst] = (oh, ow)
                C = _pad64(op.cout)
                g = ops.mbconv_geometry(WALK, n * oh * ow, C)
                assert g[0] in t["walk_rows"] and _flags(g) in t["walk_flags"], (net, op.name, g)
                if op.kind == arch.OP_DWCONV:
                    d = ops.mbconv_geometry(DWW, n * oh * ((ow + 3) // 4), C)
                    assert d[0] in t["dww_rows"] and _flags(d) in t["dww_flags"], (net, op.name, d)
                    for acc in (0, 1):
                        f = ops.mbconv_geometry(FORM, op.k, op.stride, op.pad, acc)
                        assert (op.k, op.stride, f[0]) in t["fwd"] and (op.k, op.stride, f[1], acc) in t["dgrad"]
            elif op.kind == arch.OP_SE:
                dims[op.dst] = (ih, iw)
                g = ops.mbconv_geometry(POOL, c=_pad64(op.cout), hw=ih * iw)
                assert g[1] in t["chunks"] and _flags(g) in t["pool_flags"], (net, op.name, g)
                q = ops.mbconv_geometry(SEG, m=op.cout, s=op.k)
                assert q[2] in t["nq"] and q[3] in t["sj"] and min(q[1], 2) in t["gate_tiles"], (net, op.name, q)
            elif op.kind in (arch.OP_GAVGPOOL, arch.OP_LINEAR):
                dims[op.dst] = (1, 1)
            else:
                dims[op.dst] = (ih, iw)
