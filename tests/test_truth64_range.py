"""The activation-range grid (truth_compare.RANGE) on the CPU.  The fp16 modes store every 32-channel tensor between two
layers as fp16 (or a hi/lo pair of fp16), which ends at 65504, and every other accuracy test runs on weights whose
activations stay below 11.  The gauge (truth_compare.gauge) moves the stored values along the fp16 format without changing
the function the network computes: checked here are that it really is exact (truth, fp32 torch run and C oracle bit-identical
at every grid point — so one Refs judges them all), that it has teeth (a gauge that forgets the biases or the head, or a gain
that is no power of two, moves the truth), and that the committed grid reaches what it is named after: classified from the
truth's own activations and the fp16 format alone (truth_compare.range_class), per branch and per model at least two in-range
points above k = 0, one below, and two that overflow.  CPU only; every point's truth is computed once per process."""
import numpy as np
import pytest

import torch_ref
import truth_compare as tc
from hobot_stereonet_amd import spec, weights

W, H, D = tc.SHAPE_S


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("disp", "disp_low", "cost")) and len(a["levels"]) == len(b["levels"]) \
        and all(np.array_equal(m, n) for m, n in zip(a["levels"], b["levels"]))


def test_gauge_touches_what_it_names():
    lv = tc.MULTI
    blob, table = weights.synthetic(0, lv), spec.offsets(lv)
    g = tc.gauge(blob, lv, tower=4.0, low=8.0, only_level=2)
    assert g is not blob and np.array_equal(blob, weights.synthetic(0, lv))
    ratio = {}
    for name, (off, shape) in table.items():
        n = int(np.prod(shape))
        if name == "__total__" or n == 0:
            continue
        a, b = blob[off:off + n], g[off:off + n]
        nz = a != 0
        r = np.unique(b[nz] / a[nz])
        assert r.size == 1, name
        ratio[name] = float(r[0])
    want = {n: 1.0 for n in ratio}
    want.update({"ref2.in.w": 4.0, "ref2.in.b": 4.0, "ref2.out.w": 0.25, "feat.down0.w": 8.0, "feat.down0.b": 8.0, "agg.out.w": 0.125})
    want.update({f"ref2.res{i}.{j}.b": 4.0 for i in range(spec.N_REF_RES) for j in (1, 2)})
    want.update({f"feat.down{i}.b": 8.0 for i in range(1, spec.N_DOWN)})
    want.update({f"feat.res{i}.{j}.b": 8.0 for i in range(spec.N_FEAT_RES) for j in (1, 2)})
    want.update({"feat.out.b": 8.0, **{f"agg.conv{i}.b": 8.0 for i in range(spec.N_AGG)}})
    assert ratio == want
    every = tc.gauge(blob, lv, tower=2.0)
    for k in range(lv):
        assert np.array_equal(weights.tensor(every, spec.ref_prefix(k) + ".out.w"), weights.tensor(blob, spec.ref_prefix(k) + ".out.w") * np.float32(0.5))
        assert np.array_equal(weights.tensor(every, spec.ref_prefix(k) + ".out.b"), weights.tensor(blob, spec.ref_prefix(k) + ".out.b"))


@pytest.mark.parametrize("name", list(tc.RANGE))
def test_the_truth_is_bit_identical_along_the_gauge(name):
    levels = tc.RANGE[name][0]
    blob, truth, prof = tc.range_point(name)
    base = tc.range_point(tc.RANGE_BASE[levels])[1]
    tc.assert_float64(truth)
    print(f"\n{name}: {tc.point_class(prof)}; tower A_max {prof['tower'][0]:.4g} sub {100 * prof['tower'][1]:.2f} %, "
          f"low A_max {prof['low'][0]:.4g} sub {100 * prof['low'][1]:.2f} %")
    assert _same(truth, base)
    assert np.isfinite(blob).all() and (blob != 0).sum() == (tc.range_blob(tc.RANGE_BASE[levels]) != 0).sum()    # nothing underflowed


def test_the_profile_leaves_torch_ref_as_it_was():
    before = (torch_ref.F.conv2d, torch_ref.F.conv3d, torch_ref.lrelu, torch_ref.cost_volume, torch_ref.res_block, torch_ref.refine)
    _, truth, prof = tc.range_point("S-k0")
    assert before == (torch_ref.F.conv2d, torch_ref.F.conv3d, torch_ref.lrelu, torch_ref.cost_volume, torch_ref.res_block, torch_ref.refine)
    x = tc.domain_input(W, H, D, tc.RANGE_INPUT)
    assert _same(truth, torch_ref.truth(tc.range_blob("S-k0"), x, D))          # looking at the tensors changes none
    assert set(prof["levels"]) == {0} and prof["levels"][0] == prof["tower"]
    assert set(tc.range_point("M-k0")[2]["levels"]) == set(range(tc.MULTI))
    # the base regime: nothing in the suite before this grid was within a factor of 3000 of the format's end
    assert 1.0 < prof["tower"][0] < 20.0 and 1.0 < prof["low"][0] < 20.0


@pytest.mark.parametrize("which", ["ref.in without the biases", "without the head", "a gain of 3"])
def test_teeth(which):
    x = tc.domain_input(W, H, D, tc.RANGE_INPUT)
    blob, table = weights.synthetic(0, 1), spec.offsets(1)
    base = tc.range_point("S-k0")[1]
    g = blob.copy()
    if which == "ref.in without the biases":
        tc._scale(g, table, "ref.in.w", 16.0)
        tc._scale(g, table, "ref.in.b", 16.0)
        tc._scale(g, table, "ref.out.w", 1 / 16.0)
    elif which == "without the head":
        g = tc.gauge(blob, 1, tower=16.0)
        tc._scale(g, table, "ref.out.w", 16.0)
    else:
        g = tc.gauge(blob, 1, tower=3.0, low=3.0)
    t = torch_ref.truth(g, x, D)
    diff = float(np.abs(t["disp"] - base["disp"]).max())
    print(f"\n{which}: max |d disp| {diff:.3e}")
    assert not np.array_equal(t["disp"], base["disp"])
    if which != "a gain of 3":
        assert diff > 1e-3            # a different function, not round-off
    else:
        # the same function, but not bit for bit: w * 3 and w / 3 are rounded to fp32 in the blob (2^-24 relative on
        # every weight, against a map of up to D = 96 px) — why the gains are powers of two
        assert diff < 1e-4


@pytest.mark.parametrize("levels", [1, tc.MULTI])
def test_the_fp32_checkers_are_bit_identical_along_the_gauge(oracle, levels):
    """the fp32 torch run and the C oracle at the ends of every axis and at the `both` point against k = 0: one Refs per model"""
    x, _, r = tc.range_refs(oracle, levels)
    names = [n for n, g in tc.RANGE.items() if g[0] == levels and n != tc.RANGE_BASE[levels]]
    for name in names:
        blob = tc.range_blob(name)
        with torch_ref.torch_threads():
            t32 = torch_ref.forward(blob, x, D)
        assert _same(t32, r.t32), name
        odisp, oraw, olow, omaps = oracle.forward_levels(blob, x, D)
        assert np.array_equal(odisp, r.oracle["disp"]) and np.array_equal(oraw, r.oracle["raw"]) and np.array_equal(olow, r.oracle["disp_low"]), name
        assert all(np.array_equal(m, r.oracle["levels"][k]) for k, m in enumerate(omaps, start=1)), name


def test_the_grid_reaches_both_ends_of_the_format():
    cls = {n: (tc.range_class(*tc.range_point(n)[2]["tower"]), tc.range_class(*tc.range_point(n)[2]["low"])) for n in tc.RANGE}
    for levels, tag in ((1, "S"), (tc.MULTI, "M")):
        for bi, branch in enumerate(("tower", "low")):
            pts = {n: g[1 + bi] for n, g in tc.RANGE.items() if g[0] == levels and g[2 - bi] == 0 and g[3] is None and g[1 + bi] != 0}
            inr = sorted(k for n, k in pts.items() if cls[n][bi] == "in range")
            over = sorted(k for n, k in pts.items() if cls[n][bi] == "overflows")
            print(f"\n{tag} {branch}: in range {inr}, overflows {over}, other {sorted(set(pts.values()) - set(inr) - set(over))}")
            assert len([k for k in inr if k > 0]) >= 2 and len([k for k in inr if k < 0]) >= 1 and len(over) >= 2
            assert max(inr) == tc.RANGE_TOP[branch]                      # the `top` points are where they claim to be
            axis = {(1, "tower"): tc.RANGE_TOWER_K, (1, "low"): tc.RANGE_LOW_K, (tc.MULTI, "tower"): tc.RANGE_TOWER_K_MULTI,
                    (tc.MULTI, "low"): tc.RANGE_LOW_K_MULTI}[(levels, branch)]
            assert sorted(pts.values()) == sorted(axis)
            assert {-4, tc.RANGE_TOP[branch], 14} <= set(pts.values())   # what every axis of either model has
            for n, k in pts.items():                                     # a gauge moves its own branch only
                assert cls[n][1 - bi] == "in range", n
    assert cls["S-both-top"] == ("in range", "in range")
    prof = tc.range_point("M-level2+16")[2]                              # one coarse tower alone
    assert tc.range_class(*prof["levels"][2]) == "overflows" and tc.point_class(prof) == "overflows"
    assert all(tc.range_class(*prof["levels"][k]) == "in range" for k in (0, 1, 3))
    assert tc.point_class(tc.range_point("M-level2+14")[2]) == "guard band"
    assert tc.point_class(tc.range_point("S-k0")[2]) == tc.point_class(tc.range_point("M-k0")[2]) == "in range"


def test_classification_uses_the_format_alone():
    assert tc.F16_MAX == float(np.finfo(np.float16).max) and tc.F16_MIN_NORMAL == float(np.finfo(np.float16).tiny)
    assert tc.range_class(tc.F16_MAX / 2, 0.05) == "in range" and tc.range_class(tc.F16_MAX / 2 + 1, 0.0) == "guard band"
    assert tc.range_class(10.0, 0.051) == "guard band" and tc.range_class(2 * tc.F16_MAX, 0.0) == "overflows"
    assert tc.range_class(2 * tc.F16_MAX - 1, 0.0) == "guard band"
