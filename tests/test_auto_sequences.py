"""The default precision (SN_PREC_AUTO) over a SEQUENCE of calls on one handle — the CPU side.  Every earlier test of the
1e-3 px claim judges the first call of a fresh handle; what acts from the second call on (the hysteresis, the re-entry after
SN_AUTO_CALM_CALLS calm calls, the re-calibration, the late folding of an enqueue-only call's statistic) is checked on the
GPU by tests/test_gpu_auto_sequences.py with the tools tested here:

* the frame table (truth_compare.SEQ_*): nine frames at 160x96 D=96 under a single-scale and a hierarchical seed-0 model,
  each with its float64 truth and the truth's own refinement residual sum_k 2^k mean |D_k r_k| — the premises that make a
  sequence of them able to judge anything are asserted here;
* truth_compare.replay: what a handle reported call by call against the pure state machine (sn_auto_*) — three wrong
  trajectories must be flagged and a correct one must not.
No GPU."""
import os
import re

import numpy as np
import pytest

import truth_compare as tc
from hobot_stereonet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()


def _define(name):
    return float(re.search(rf"#define\s+{name}\s+([0-9.eE+-]+)", HEADER).group(1))


BUDGET, REENTRY, CALM = _define("SN_AUTO_BUDGET_PX"), _define("SN_AUTO_REENTRY"), int(_define("SN_AUTO_CALM_CALLS"))
MODELS = list(tc.SEQ_LEVELS)


def test_the_frame_lists_are_the_committed_ones():
    assert set(tc.SEQ_CALLS) | set(tc.SEQ_ROTATED) == set(tc.SEQ_KINDS) and len(tc.SEQ_KINDS) == 9
    kinds = [k in tc.SEQ_CALM for k in tc.SEQ_CALLS]
    # calm x2, hard, hard, calm x9, hard, calm, noise, hard
    assert kinds == [True] * 2 + [False] * 2 + [True] * 9 + [False, True, False, False] and len(tc.SEQ_CALLS) == 17
    assert [k in tc.SEQ_HARD for k in tc.SEQ_CALLS] == [False] * 2 + [True] * 2 + [False] * 9 + [True, False, False, True]
    assert tc.SEQ_CALLS[15] == "noise" and tc.SEQ_CALLS[0] == "zero" and tc.SEQ_CALLS[12] != tc.SEQ_CALLS[0]
    assert all(f in tc.SEQ_ROTATED for f in tc.SEQ_ROTATIONS) and tc.SEQ_ROTATIONS == ("zero", "tex4", "min")
    assert all(g in (2.0, 4.0, 8.0) for g in tc.SEQ_GAIN.values())
    xs = [tc.seq_input(f) for f in tc.SEQ_KINDS]
    assert all(x.shape == (6, 96, 160) and x.dtype == np.int8 for x in xs)
    assert len({x.tobytes() for x in xs}) == 9


@pytest.mark.parametrize("model", MODELS)
def test_premises_of_the_frame_table(oracle, model):
    """Every truth finite; the oracle within X3_TOL of it on every frame (else the frame cannot judge a mode); the residuals
    spread over a factor of 3 or more; every calm frame, and `noise`, below SN_AUTO_REENTRY = 0.8 of the smallest hard
    frame's residual (the hysteresis band: a limit between them lets the calm ones count as calm)."""
    w, h, d = tc.SHAPE_S
    blob, levels = tc.seq_blob(model), tc.SEQ_LEVELS[model]
    res = {}
    for f in tc.SEQ_KINDS:
        x, t, lv, r = tc.seq_point(model, f)
        tc.assert_float64(t)
        for k, v in t.items():
            assert all(np.isfinite(m).all() for m in (v if k == "levels" else [v])), (f, k)
        e = tc.err(oracle.forward(blob, x, d)[0], t["disp"])
        print(f"{model} gain {tc.SEQ_GAIN[model]:g} {f:<8} residual {r:.4f} px, levels {['%.4f' % v for v in lv]}, oracle E/M/S {tc.fmt(e)}")
        assert e[0] < tc.X3_TOL, (f, e)
        assert len(lv) == levels and all(v > 0 for v in lv) and abs(r - sum(v * 2 ** k for k, v in enumerate(lv))) < 1e-12
        res[f] = r
    assert tc.seq_point(model, "zero")[1] is tc.seq_point(model, "zero")[1]            # computed once
    assert max(res.values()) >= 3.0 * min(res.values())
    hard = min(res[f] for f in tc.SEQ_HARD)
    assert REENTRY == 0.8
    for f in tc.SEQ_CALM + ("noise",):
        assert res[f] < REENTRY * hard, (f, res[f], hard)
    assert res["zero"] == min(res.values())                    # the calmest frame is the one the first self-check sees


def test_the_truth_residual_is_the_table_of_the_record():
    """mean |D r| of the single-scale model at head gain 1 (the figures the sequence tests were planned with), and their
    linearity in the head gain"""
    import torch_ref
    from hobot_stereonet_amd import weights
    w, h, d = tc.SHAPE_S
    want = {"zero": 0.265, "noise": 0.44, "checker": 0.66, "max": 0.81, "step": 0.86, "min": 0.90}
    for f, v in want.items():
        moved = []
        torch_ref.truth(weights.synthetic(0, 1), tc.seq_input(f), d, moved)
        lv, r = tc.truth_residual(moved, h, w)
        assert len(moved) == 1 and moved[0].shape == (96, 160) and abs(r - v) < 0.006, (f, r)
        assert abs(tc.seq_point("single", f)[3] - tc.SEQ_GAIN["single"] * r) < 0.02 * tc.SEQ_GAIN["single"] * r


# ---- replay --------------------------------------------------------------------------------------------------------------------
def _handle(frames, limit_rule, calm_calls=CALM, skip_repeat=(), scale=None):
    """A handle of the default precision in plain Python, after the header's text (not the library's code): frames =
    [(residual in F16, residual in F16X3, EPE of the F16 map against the F16X3 map)] per call -> its sn_get_refine_stats after
    every call.  skip_repeat: calls that return the F16 map although the rule demands the repeat; calm_calls: consecutive
    calm calls before the re-entry; scale = (call, factor): that call REPORTS its residual times factor."""
    mode, calm, slope, calibrated, switches, reruns, check = "f16", 0, 0.0, False, 0, 0, (-1.0, -1.0)
    out = []
    for i, (r16, r3, epe) in enumerate(frames):
        ran = mode
        seen = r16 if mode == "f16" else r3
        if mode == "f16" and not calibrated:
            check, slope, calibrated = (epe, r16), (epe / r16 if r16 > 1e-6 else 0.0), True
        lim = limit_rule(slope)
        reported = seen
        if mode == "f16":
            if seen > lim:
                mode, calm, switches = "f16x3", 0, switches + 1
                if i not in skip_repeat:
                    ran, reruns, reported = "f16x3", reruns + 1, r3
        elif seen < REENTRY * lim:
            calm += 1
            if calm >= calm_calls:
                mode, calm, switches, calibrated = "f16", 0, switches + 1, False
        else:
            calm = 0
        rec = {"residual_px": reported, "observed_px": seen, "precision_last": ran, "reruns": reruns, "switches": switches,
               "selfcheck_epe_px": check[0], "selfcheck_residual_px": check[1], "precision_selected": mode}
        if scale and scale[0] == i:
            rec["residual_px"] = rec["observed_px"] = seen * scale[1]
        out.append(rec)
    return out


def _limit_rule(env):
    return lambda slope: env if not slope > 0 else min(env, BUDGET / slope)


def _frames(env):
    """the committed call list with residuals placed around a limit of 0.9 envelopes: calm 0.5 of it, noise 0.7, hard 1.3; the
    F16X3 residual a little off the F16 one; slope = budget over 0.9 envelopes on every frame"""
    lim = 0.9 * env
    level = {f: 0.5 for f in tc.SEQ_CALM}
    level.update({f: 1.3 for f in tc.SEQ_HARD}, noise=0.7, checker=0.9)
    out = []
    for i, f in enumerate(tc.SEQ_CALLS):
        r16 = lim * level[f] * (1.0 + 0.01 * i)
        out.append((r16, r16 * (1.0 + 1e-4), BUDGET / lim * r16))
    return out


@pytest.mark.parametrize("levels", (1, 4))
def test_a_correct_trajectory_replays_clean_and_is_live(levels):
    env = api.load_library().sn_auto_envelope_px(levels)
    traj = _handle(_frames(env), _limit_rule(env))
    assert tc.replay(traj, levels) == []
    assert [r["precision_last"] for r in traj] == ["f16"] * 2 + ["f16x3"] * 10 + ["f16", "f16x3", "f16x3", "f16x3", "f16x3"]
    assert traj[-1]["switches"] == 3 and traj[-1]["reruns"] == 2
    assert tc.trajectory_is_live(traj) == (2, 12, 13)
    assert tc.trajectory_is_live(traj[:12]) == (2, None, None)


@pytest.mark.parametrize("levels", (1, 4))
def test_replay_flags_three_wrong_handles(levels):
    env = api.load_library().sn_auto_envelope_px(levels)
    frames, rule = _frames(env), _limit_rule(env)
    # 1. the repeat skipped: call 2 returns its F16 map
    bad = tc.replay(_handle(frames, rule, skip_repeat=(2,)), levels)
    assert bad and bad[0][0] == 2 and "demanded the repeat" in bad[0][1], bad
    # 2. re-entry after 7 calm calls: call 10 is the seventh calm one, call 11 then runs in F16
    bad = tc.replay(_handle(frames, rule, calm_calls=CALM - 1), levels)
    assert bad and bad[0][0] == 10 and "extra switch" in bad[0][1], bad
    assert any(i == 11 and "re-entry after 7 calm calls" in m for i, m in bad), bad
    # 3. one call's residual reported times b/a (a pending statistic of an a-pair call divided into a b-pair call's sums):
    #    a calm call reads as hard (a missing switch), a hard call as calm (an extra one)
    bad = tc.replay(_handle(frames, rule, scale=(1, 3.0)), levels)
    assert bad and bad[0][0] == 1 and any(i == 1 and "missing switch" in m for i, m in bad), bad
    bad = tc.replay(_handle(frames, rule, scale=(2, 1.0 / 3.0)), levels)
    assert bad and bad[0][0] == 2 and any(i == 2 and "extra switch" in m for i, m in bad), bad
    # 4. a re-entry without a new self-check: call 12 keeps the first call's self-check values
    traj = _handle(frames, rule)
    for r in traj[12:]:
        r["selfcheck_epe_px"], r["selfcheck_residual_px"] = traj[0]["selfcheck_epe_px"], traj[0]["selfcheck_residual_px"]
    bad = tc.replay(traj, levels)
    assert bad and bad[0][0] == 12 and "without a new self-check" in bad[0][1], bad


def test_replay_follows_the_measured_slope():
    """a trajectory that is right under one self-check slope is wrong under another: the limit replay uses is the handle's own"""
    env = api.load_library().sn_auto_envelope_px(1)
    frames = _frames(env)
    traj = _handle(frames, _limit_rule(env))
    steep = [dict(r, selfcheck_epe_px=4.0 * r["selfcheck_epe_px"]) for r in traj]       # limit 0.225 envelopes: every call is outside
    bad = tc.replay(steep, 1)
    assert bad and bad[0][0] == 0 and "demanded the repeat" in bad[0][1]
