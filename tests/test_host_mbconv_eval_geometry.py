"""The cases of tests/test_gpu_mbconv_eval_ops.py reach every launch branch of the eval kernels they test.

No GPU: the case lists are fed through `spk_op_mbconv_eval_geometry`, which reports what the launchers' own helpers
choose (`spk_se_fc1_ch`, `spk_se_ipb`, `spk_se_fc2_stage`, `spk_se_scale_grid`, `spk_stem3_gt` of csrc/effnet.hip,
`spk_conv_narrow_cfg` and `spk_conv_padc_flavour` of csrc/conv_igemm.hip - the functions the launches call).  Also here,
because it needs no GPU either: the number of elements the BOUNDED tests leave out next to a Hardswish kink."""

import test_gpu_mbconv_eval_ops as T
from sykepic_hip import ops

SE, SCALE, STEM3, PADC = 0, 1, 2, 3


def _se(case):
    c, sq, kind, n, chunks, hw = case
    return ops.mbconv_eval_geometry(SE, n, chunks, c, sq)


def test_se_cases_reach_every_branch():
    for cases in (T.SE_CASES, T.SE_EXACT_CASES):
        g = [_se(case) for case in cases]
        assert {q[0] for q in g} == {0, 1, 2, 3, 4, 8}, "a CH instantiation of se_fc1 (or its run-time loop) is not reached"
        assert any(q[0] == 0 and q[1] > 0 for q in g), "run-time loop: no case with chunks % 4 != 0"
        assert any(q[0] == 0 and q[1] == 0 for q in g), "run-time loop: no case with chunks % 4 == 0"
        assert any(q[2] < 8 for q in g) and any(q[2] == 8 for q in g), "image tail nim < 8 / full block"
        assert any(q[7] > 1 and q[2] < 8 for q in g), "no case with a full block AND a tail block"
        assert any(q[3] > 0 for q in g) and any(q[3] == 0 for q in g), "hidden tail sq % 4"
        assert any(q[4] > 1 for q in g) and any(q[4] == 1 for q in g), "second staging pass of se_fc2 (sq * 8 > 1024)"
        assert any(q[5] > 1 and q[6] != 256 for q in g), "c > 256 with c % 256 != 0"
        assert any(q[5] == 1 and q[6] != 256 for q in g), "c < 256"
        # every batch size, every pool-partial row count, every hw of the lists is used
        assert {case[3] for case in cases} == set(T.SE_N) and {case[4] for case in cases} == set(T.SE_CHUNKS)
        assert {(case[0], case[1]) for case in cases} == {(c, sq) for (c, sq, _) in T.SE_LAYERS}
    assert {case[5] for case in T.SE_CASES} == set(T.SE_HW)
    assert {case[2] for case in T.SE_CASES} == {0, 1}
    for case in T.SE_EXACT_CASES + [T.SE_SCALE_CAP_CASE]:
        assert case[5] & (case[5] - 1) == 0 and case[2] == 1, "exact: hw a power of two, ReLU / Hardsigmoid gates"


def test_se_scale_grid_cap_is_reached():
    c, sq, kind, n, chunks, hw = T.SE_SCALE_CAP_CASE
    g = ops.mbconv_eval_geometry(SCALE, n, hw, c)
    assert g[0] < g[1], f"the grid of se_scale is not capped: {g[:2]}"
    for (c, sq, kind, n, chunks, hw) in T.SE_CASES:
        g = ops.mbconv_eval_geometry(SCALE, n, hw, c)
        assert g[0] == g[1]          # the small cases run uncapped: both forms are tested


def test_stem3_cases_reach_every_gt():
    for cases in (T.STEM3_EXACT_CASES, T.STEM3_RANDOM_CASES):
        gts = {}
        for (n, h, w, cout, act) in cases:
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            gts.setdefault(ops.mbconv_eval_geometry(STEM3, ho, wo, cout)[0], set()).add((ho, wo))
        assert set(gts) == {0, 4, 5, 6}
        for gt, sizes in gts.items():
            assert any(wo % 4 for _, wo in sizes), f"GT {gt}: no wo tail"
            assert any(ho % 2 for ho, _ in sizes), f"GT {gt}: no block with a single output row"
        assert {c[3] for c in cases} == set(T.STEM3_COUTS) and {(c[1], c[2]) for c in cases} == set(T.STEM3_SIZES)
        assert len({c[3] for c in cases if ops.mbconv_eval_geometry(STEM3, 1, 1, c[3])[0] == 0}) == 3   # 16, 24, 64


def _padc_reached(cases):
    got = set()
    for (cin, cout, n, h, w, res, split, act, gated) in cases:
        if not (gated or cin % 64 or cout % 64):
            continue
        for cfg, fl in T.GRID:
            g = ops.mbconv_eval_geometry(PADC, cfg, fl, T.pad64(cout), split + 2 * gated)
            # the file's own refusal rule is the launcher's
            assert (g[1] >= 0) == T.expected_to_run(cfg, fl, cin, cout, bool(split), bool(gated)), (cin, cout, cfg, fl)
            if g[1] >= 0:
                got.add((g[0], g[1], split, gated))
    return got


def test_padded_conv_cases_reach_every_instantiation():
    # everything the launcher can instantiate on the padded / gated path: every tile it narrows to x DMA argument
    every = set()
    for cout_p in (64, 128, 256):
        for cfg in range(7):
            for fl in range(7):
                for d in range(4):
                    g = ops.mbconv_eval_geometry(PADC, cfg, fl, cout_p, d)
                    if g[1] >= 0:
                        every.add((g[0], g[1], d & 1, d >> 1))
    assert len(every) == (7 + 6) * 3 + (7 + 6) * 1      # 7 tiles (6 with split weights) x {0, 2, 4} / gated {0}
    for cases in (T.PAD_EXACT_CASES, T.PAD_RANDOM_CASES):
        assert _padc_reached(cases) == every, sorted(every - _padc_reached(cases))
        # the shapes: every (cin, cout) with and without split weights, every M, shortcut and none, every activation
        assert {(c[0], c[1]) for c in cases if not c[8]} == set(T.PAD_PAIRS)
        assert {(c[0], c[1]) for c in cases if c[8]} == set(T.GATED_PAIRS)
        for gated in (0, 1):
            sub = [c for c in cases if c[8] == gated]
            assert {c[2:5] for c in sub} == set(T.PAD_SHAPES) and {c[5] for c in sub} == {0, 1}
            assert {(c[0], c[1], c[6]) for c in sub} == {(a, b, s) for (a, b) in (T.GATED_PAIRS if gated else T.PAD_PAIRS)
                                                           for s in (0, 1)}
    assert {c[7] for c in T.PAD_EXACT_CASES} == {T.ACT_NONE, T.ACT_RELU}
    for gated in (0, 1):
        assert {c[7] for c in T.PAD_RANDOM_CASES if c[8] == gated} == {T.ACT_NONE, T.ACT_RELU, T.ACT_SILU, T.ACT_HSWISH}
    # gated: a tile that holds rows of more than one image, and a last tile that runs past M
    assert any(c[8] and c[2] > 1 and c[3] * c[4] % 64 for c in T.PAD_EXACT_CASES)


def test_kink_exclusions_stay_under_a_tenth_of_a_percent():
    """The float64 references of the Hardswish cases: elements within 2^-16 A' of +-3."""
    for case in T.PAD_RANDOM_CASES:
        if case[7] == T.ACT_HSWISH:
            o = T.pad_conv_reference(case, exact=False)
            keep = T.fp16_bound(o["pre"], o["mag"], case[7])[2]
            assert int((~keep).sum()) <= keep.numel() // 1000, (case, int((~keep).sum()), keep.numel())
    for case in T.STEM3_RANDOM_CASES:
        if case[4] == T.ACT_HSWISH:
            o = T.stem3_reference(case, exact=False)
            keep = T.fp16_bound(o["pre"], o["mag"], case[4])[2]
            assert int((~keep).sum()) <= keep.numel() // 1000, (case, int((~keep).sum()), keep.numel())


def test_exact_references_meet_their_preconditions():
    """Sum of |terms| < 2^24 and |value| within fp16's integer range, for every exact case, before any GPU is asked."""
    for case in T.PAD_EXACT_CASES:
        o = T.pad_conv_reference(case, exact=True)
        ref = T.act64(o["pre"], case[7])
        assert float(o["mag"].max()) < T.TWO24 and float(ref.abs().max()) <= (1024 if case[8] else 2048), case
        assert bool((ref.half().double() == ref).all()), case
    assert float(T.folded_stem_scale(T.torch.tensor([255.0]))[0]) == 1.0
