"""The input-domain grid (truth_compare.DOMAIN) on the CPU: 32 small points that reach the edges the full-size truth64 grid
never does — a near one-hot and a flat soft-argmin, images at the int8 limits, a final relu that clamps, a single-plane
cost volume (D = 16), 1x1 low-resolution maps, W or H below 16.  Checked here: the points really reach the edges they are
named after, the CPU checkers stay inside the project's bounds there, and the judging function for a result that claims to
be fp32-class (truth_compare.class_failures, with the unchanged factors of tests/test_gpu_truth64.py) tells three subtly
wrong networks from round-off at these shapes — so that a HIP mode judged on this grid cannot pass vacuously.  CPU only;
every reference of a grid point is computed once per process."""
import contextlib

import numpy as np
import pytest
import torch

import truth_compare as tc

_desc = {}


def _describe(oracle, name):
    if name not in _desc:
        _desc[name] = tc.describe(tc.domain_point(oracle, name)[3].truth)
    return _desc[name]


def test_the_grid_is_complete_and_small():
    g = tc.DOMAIN
    assert len(g) == 32 and len({(v[:4], repr(v[4]), v[5]) for v in g.values()}) == 32
    assert all(w <= 250 and h <= 250 and w * h <= 160 * 96 for w, h, *_ in g.values())
    assert len(tc.D16) == 5 and {g[n][:2] for n in tc.D16} == {(96, 64), (16, 16), (8, 8), (1, 1)}
    assert tc.MIN_STAGE_VALUES == 24
    x = tc.domain_input(6, 4, 16, "checker")
    assert x[0, 0, 0] == 127 and x[0, 0, 1] == -128 and x[0, 1, 0] == -128 and (x == x[0]).all()
    x = tc.domain_input(6, 4, 16, "step")
    assert (x[:, :, :3] == 127).all() and (x[:, :, 3:] == -128).all()
    x = tc.domain_input(160, 96, 96, "noise")
    assert x.min() == -128 and x.max() == 127 and abs(float(x.mean())) < 1.0


def test_scaled_multiplies_one_layer():
    from hobot_stereonet_amd import spec, weights
    blob = weights.synthetic(0, spec.MULTI_LEVELS)
    out = tc.scaled(blob, "agg.out", 16.0, spec.MULTI_LEVELS)
    assert out is not blob and np.array_equal(blob, weights.synthetic(0, spec.MULTI_LEVELS))
    for suffix in (".w", ".b"):
        assert np.array_equal(weights.tensor(out, "agg.out" + suffix), weights.tensor(blob, "agg.out" + suffix) * np.float32(16))
    changed = np.flatnonzero(out != blob)
    off = spec.offsets(spec.MULTI_LEVELS)["agg.out.w"][0]
    assert changed.min() >= off and changed.max() < off + 32 * 27 + 1


@pytest.mark.parametrize("name", list(tc.DOMAIN))
def test_checkers_stay_inside_the_bounds_at_every_grid_point(oracle, name):
    """E_ref < X3_TOL (a checker that is itself outside the fp32-class bound could not judge it), every reference finite,
    and the two CPU checkers pass the criteria they set for the GPU (each is within the larger of the two by construction:
    this is the plumbing of class_failures at every shape of the grid, the stages below MIN_STAGE_VALUES included)."""
    blob, x, x_other, r = tc.domain_point(oracle, name)
    w, h, d, levels, wk, kind = tc.DOMAIN[name]
    peak, zeros = _describe(oracle, name)
    print(f"\n{name}: {w}x{h} D={d} levels={levels}: peak probability {peak:.3f}, zero pixels {100 * zeros:.1f} %, E_ref {r.E_ref:.2e} "
          f"M_ref {r.M_ref:.2e}; refs " + "  ".join(f"{k} {tc.fmt(v)}" for k, v in r.ref.items() if k != "disp")
          + f"; {sum(r.seconds.values()):.2f} s")
    assert r.E_ref < tc.X3_TOL
    assert not np.array_equal(x, x_other)
    tc.assert_float64(r.truth)
    for k, v in r.truth.items():
        assert all(np.isfinite(m).all() for m in (v if k == "levels" else [v])), k
    assert r.truth["disp"].min() >= 0 and r.oracle["raw"].min() >= 0
    t32 = tc.forward_as_stages(r.t32)
    assert tc.class_failures(r, t32, tc.FP32_FACTOR) == []
    orc = {"disp": r.oracle["disp"], "disp_low": r.oracle["disp_low"], **{f"level{k}": m for k, m in r.oracle["levels"].items()}}
    assert tc.class_failures(r, orc, tc.FP32_FACTOR) == []


def test_cost_sharpness_reaches_both_ends(oracle):
    """agg.out x16 / x64: near one-hot; x1/16 and the all-zero image: flat (uniform over the 6 planes is 1/6); act_scale 4
    in between but well above the 0.47 of the default weights."""
    for name in tc.SHARP:
        assert _describe(oracle, name)[0] > 0.9, (name, _describe(oracle, name))
    for name in tc.FLAT:
        assert _describe(oracle, name)[0] < 0.2, (name, _describe(oracle, name))
    for name in tc.ACT4:
        assert _describe(oracle, name)[0] > 0.75, (name, _describe(oracle, name))
    for name in tc.ACT4_DEEP:
        assert _describe(oracle, name)[0] > 0.6, (name, _describe(oracle, name))


def test_the_final_relu_clamps(oracle):
    for name in tc.CLAMPED:
        assert _describe(oracle, name)[1] > 0, name
    for name in tc.D16:
        r = tc.domain_point(oracle, name)[3]
        assert _describe(oracle, name)[1] > 0.5, (name, _describe(oracle, name))
        for low in (r.truth["disp_low"], r.oracle["disp_low"], r.t32["disp_low"]):      # one plane: the soft-argmin is 0 * 1
            assert not low.any(), name


# ---- teeth: three networks that are wrong at an edge of the domain -----------------------------------------------------------
def _replicated_cost_volume(fl, fr, dl):
    """the cost volume filled by edge replication instead of zeros where x < d"""
    _, c, h, w = fl.shape
    cv = torch.zeros(1, c, dl, h, w, dtype=fl.dtype)
    for d in range(dl):
        idx = (torch.arange(w) - d).clamp(min=0)
        cv[:, :, d] = fl - fr[..., idx]
    return cv


def _aggregate_open_ends(blob, fl, fr, dl):
    """the output conv as a contraction over dz whose taps outside the volume are still counted (they read the nearest
    plane) while the first and the last plane go without the conv's bias"""
    import torch.nn.functional as F
    import torch_ref
    from hobot_stereonet_amd import spec
    x, dt = torch_ref.cost_volume(fl, fr, dl), fl.dtype
    for i in range(spec.N_AGG):
        x = torch_ref.lrelu(F.conv3d(x, torch_ref._t(blob, f"agg.conv{i}.w", dt), torch_ref._t(blob, f"agg.conv{i}.b", dt), padding=1))
    b = torch_ref._t(blob, "agg.out.b", dt)
    xp = F.pad(F.pad(x, (1, 1, 1, 1, 0, 0)), (0, 0, 0, 0, 1, 1), mode="replicate")
    cost = F.conv3d(xp, torch_ref._t(blob, "agg.out.w", dt), b)[:, 0]
    cost[:, 0] -= b
    if dl > 1:
        cost[:, dl - 1] -= b
    return cost


@contextlib.contextmanager
def _variant(monkeypatch, which):
    import torch_ref
    with monkeypatch.context() as m:
        if which == "replicated cost volume":
            m.setattr(torch_ref, "cost_volume", _replicated_cost_volume)
        elif which == "open volume ends":
            m.setattr(torch_ref, "aggregate", _aggregate_open_ends)
        elif which == "fp16 disp_low":
            orig, calls = torch_ref.F.interpolate, [0]

            def interpolate(x, *a, **k):        # the first upsample of a forward pass takes the soft-argmin map
                calls[0] += 1
                return orig(x.to(torch.float16).to(x.dtype) if calls[0] == 1 else x, *a, **k)
            m.setattr(torch_ref.F, "interpolate", interpolate)
        else:
            raise ValueError(which)
        yield


# the grid points each variant is run at: where its error is smallest against the checkers' own (narrow maps where most
# columns have x < d; a single plane and a deep volume; the sharpest and the flattest soft-argmin) and one in the middle
TEETH = {"replicated cost volume": ("S-aggx64", "S-agg/16", "16x250-d48", "17x16-d32", "48x32-d256"),
         "open volume ends": ("S-aggx64", "S-agg/16", "P-aggx16", "96x64-d16", "5x3-d32"),
         "fp16 disp_low": ("S-aggx64", "S-agg/16", "S-max", "Sm-act4", "33x47-d64")}


@pytest.mark.parametrize("which", list(TEETH))
def test_the_criteria_catch_a_subtly_wrong_network(oracle, monkeypatch, which):
    """fp32 torch_ref.forward with one deliberate error, judged as a result that claims to be fp32-class
    (class_failures, FP32_FACTOR): reported as failing at one or more grid points, and — so that this is the criterion and
    not noise — the unmodified run passes at the same points (test_checkers_stay_inside_the_bounds_at_every_grid_point)."""
    import torch_ref
    caught = {}
    for name in TEETH[which]:
        blob, x, _, r = tc.domain_point(oracle, name)
        d = tc.DOMAIN[name][2]
        with _variant(monkeypatch, which), torch_ref.torch_threads():
            res = torch_ref.forward(blob, x, d)
        bad = tc.class_failures(r, tc.forward_as_stages(res), tc.FP32_FACTOR)
        print(f"\n{which} at {name}: E/M/S of the final map {tc.fmt(tc.err(res['disp'], r.truth['disp']))} (E_ref {r.E_ref:.2e}): "
              + ("; ".join(bad) if bad else "not caught"))
        if bad:
            caught[name] = bad
        with torch_ref.torch_threads():                             # the patch is gone: the fp32 run is the checker's again
            assert np.array_equal(torch_ref.forward(blob, x, d)["disp"], r.t32["disp"])
    assert caught, f"{which}: no grid point of {TEETH[which]} catches it"
