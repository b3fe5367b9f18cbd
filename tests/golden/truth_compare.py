"""Judging a disparity map (or any stage of the network) against the float64 truth (torch_ref.truth) — shared by
tests/test_truth64.py (what the CPU checkers themselves are worth), tests/test_gpu_truth64.py (every precision mode
of the HIP path) and the two files that carry both across the input domain (tests/test_truth64_domain.py on the CPU,
tests/test_gpu_truth64_domain.py on the GPU: DOMAIN below is their grid, class_failures their judge).  Nothing here looks
at a HIP result to set a bound: E_ref / M_ref come from the two CPU fp32 implementations (the C oracle and the fp32 torch
run) on the same input, and there is no exclusion mask.

    E(a) = mean |a - truth|      M(a) = max |a - truth|      S(a) = mean (a - truth)   (signed: the coherent part)
"""
from __future__ import annotations

import time

import numpy as np

import torch_ref
from hobot_stereonet_amd import spec, synth, weights

BUDGET = 1e-3          # px: the project's bound on the mean error of a full-size map (north star; F16_TOL)
X3_TOL = 2e-4          # px: what "fp32-class" has promised for SN_PREC_F16X3 since round 4
FP32_FACTOR = 3.0      # a third fp32 summation order next to the two CPU ones (they differ by 1.4x from each other)
X3_FACTOR = 4.0        # 22-bit split operands: unit round-off 4x that of fp32's 24 bits
# The "factor x the CPU checkers' own error" criteria (stage_failures, fp32_class_failures) are statistics: 24 values is
# the smallest count they have been applied to (the 3x8 low-resolution map of 124x38).  A stage with fewer values is
# still compared on every element, but against the absolute bounds of tests/test_gpu_parity.py (small_failures).
MIN_STAGE_VALUES = 24


def err(a, t):
    """-> (E, M, S) of `a` against the truth `t`, in float64, over EVERY element"""
    d = np.asarray(a, np.float64) - np.asarray(t, np.float64)
    assert d.shape == np.asarray(t).shape, (d.shape, np.asarray(t).shape)
    return float(np.abs(d).mean()), float(np.abs(d).max()), float(d.mean())


def level_maps(r):
    """torch_ref.forward's `levels` (levels-1 .. 0) -> {k: map} of the COARSE levels k = 1 .. levels-1"""
    lv = r["levels"]
    return {len(lv) - 1 - i: m for i, m in enumerate(lv[:-1])}


class Refs:
    """One input's float64 truth, C-oracle result and fp32 torch result, and the error of the two fp32 checkers:
    ref[stage] = (E_ref, M_ref) = the larger of the two checkers' E and of their M at that stage (cost and the feature
    maps: the fp32 torch run alone — the oracle's forward does not return them)."""

    def __init__(self, oracle, blob, x, d):
        t0 = time.time()
        self.truth = torch_ref.truth(blob, x, d)
        t1 = time.time()
        with torch_ref.torch_threads():
            self.t32 = torch_ref.forward(blob, x, d)
        t2 = time.time()
        odisp, oraw, olow, omaps = oracle.forward_levels(blob, x, d)
        self.seconds = {"truth": t1 - t0, "torch32": t2 - t1, "oracle": time.time() - t2}
        self.oracle = {"disp": odisp, "raw": oraw, "disp_low": olow, "levels": {k: m for k, m in enumerate(omaps, start=1)}}
        self.levels = level_maps(self.truth)                 # {k: float64 map}
        t32_levels = level_maps(self.t32)
        self.e_oracle = {"disp": err(odisp, self.truth["disp"]), "disp_low": err(olow, self.truth["disp_low"])}
        self.e_t32 = {k: err(self.t32[k], self.truth[k]) for k in ("disp", "disp_low", "cost", "fl", "fr")}
        for k, m in self.levels.items():
            self.e_oracle[f"level{k}"] = err(self.oracle["levels"][k], m)
            self.e_t32[f"level{k}"] = err(t32_levels[k], m)
        self.ref = {}
        for k, e in self.e_t32.items():
            o = self.e_oracle.get(k, e)
            self.ref[k] = (max(e[0], o[0]), max(e[1], o[1]))

    @property
    def E_ref(self):
        return self.ref["disp"][0]

    @property
    def M_ref(self):
        return self.ref["disp"][1]

    def stage_truth(self, stage):
        """the truth of a stage under the names sn_dbg_read uses"""
        if stage.startswith("level"):
            return self.levels[int(stage[5:])]
        return self.truth[{"feat_l": "fl", "feat_r": "fr"}.get(stage, stage)]

    def stage_ref(self, stage):
        return self.ref[{"feat_l": "fl", "feat_r": "fr"}.get(stage, stage)]


def fp32_class_failures(a, truth, e_ref, m_ref, factor):
    """Assertions 2 and 4 on a final map that claims to be fp32-class: E <= factor * E_ref, M <= factor * M_ref
    (another summation order, not a lost bit) and |S| <= E_ref (round-off is not coherent; a lost operand bit is).
    -> list of the conditions missed (empty: passes)"""
    e, m, s = err(a, truth)
    bad = []
    if not np.isfinite(np.asarray(a)).all():
        bad.append("not finite")
    if not e <= factor * e_ref:
        bad.append(f"mean {e:.3e} > {factor:g} x E_ref {e_ref:.3e}")
    if not m <= factor * m_ref:
        bad.append(f"max {m:.3e} > {factor:g} x M_ref {m_ref:.3e}")
    if not abs(s) <= e_ref:
        bad.append(f"|signed mean| {abs(s):.3e} > E_ref {e_ref:.3e}")
    return bad


def stage_failures(a, truth, ref, factor):
    """One intermediate stage against its truth: E and M within `factor` of the CPU fp32 checkers' own at that stage"""
    e, m, _ = err(a, truth)
    bad = []
    if not np.isfinite(np.asarray(a)).all():
        bad.append("not finite")
    if not e <= factor * ref[0]:
        bad.append(f"mean {e:.3e} > {factor:g} x {ref[0]:.3e}")
    if not m <= factor * ref[1]:
        bad.append(f"max {m:.3e} > {factor:g} x {ref[1]:.3e}")
    return bad


def fmt(e):
    return f"{e[0]:.2e}/{e[1]:.2e}" if len(e) == 2 else f"{e[0]:.2e}/{e[1]:.2e}/{e[2]:+.1e}"


def assert_float64(r):
    """every array torch_ref.forward(..., torch.float64) returns is float64"""
    for k, v in r.items():
        for m in (v if k == "levels" else [v]):
            assert m.dtype == np.float64, (k, m.dtype)



# ---- the input domain (tests/test_truth64_domain.py, tests/test_gpu_truth64_domain.py) -------------------------------------
def scaled(blob, layer, gain, levels):
    """-> a copy of `blob` with the weights and the bias of `layer` multiplied by `gain`"""
    out = blob.copy()
    table = spec.offsets(levels)
    for suffix in (".w", ".b"):
        off, shape = table[layer + suffix]
        n = int(np.prod(shape))
        out[off:off + n] *= np.float32(gain)
    return out


def describe(truth):
    """-> (mean over the low-resolution pixels of the largest softmax probability of -cost, share of the pixels of `disp`
    that are exactly zero): how sharp the soft-argmin is and how much the final relu clamps"""
    c = -np.asarray(truth["cost"], np.float64)
    p = np.exp(c - c.max(0, keepdims=True))
    p /= p.sum(0, keepdims=True)
    return float(p.max(0).mean()), float((truth["disp"] == 0).mean())


SHAPE_S, SHAPE_P = (160, 96, 96), (96, 64, 256)
MULTI = spec.MULTI_LEVELS
# name: (w, h, D, levels, weights, input); weights = dict(act_scale, head_gain, agg_out) over seed 0, input = a seed of
# synth.model_input_i8 or the name of a pattern (domain_input)
DOMAIN = {}
for _n, _shape, _lv, _wk in (("S-act0.5", SHAPE_S, 1, {"act_scale": 0.5}), ("S-act2", SHAPE_S, 1, {"act_scale": 2.0}), ("S-act4", SHAPE_S, 1, {"act_scale": 4.0}),
                             ("S-agg/16", SHAPE_S, 1, {"agg_out": 1 / 16}), ("S-aggx16", SHAPE_S, 1, {"agg_out": 16.0}), ("S-aggx64", SHAPE_S, 1, {"agg_out": 64.0}),
                             ("P-aggx16", SHAPE_P, 1, {"agg_out": 16.0}), ("P-act4", SHAPE_P, 1, {"act_scale": 4.0}),
                             ("Sm-act4", SHAPE_S, MULTI, {"act_scale": 4.0}), ("Sm-act2-g8", SHAPE_S, MULTI, {"act_scale": 2.0, "head_gain": 8.0})):
    DOMAIN[_n] = (*_shape, _lv, _wk, 4)
for _n, _lv, _wk, _in in (("S-max", 1, {}, "max"), ("S-min", 1, {}, "min"), ("S-zero", 1, {}, "zero"), ("S-noise", 1, {}, "noise"),
                          ("S-checker", 1, {}, "checker"), ("S-step", 1, {}, "step"), ("Sm-noise", MULTI, {}, "noise"),
                          ("S-noise-g8", 1, {"head_gain": 8.0}, "noise")):
    DOMAIN[_n] = (*SHAPE_S, _lv, _wk, _in)
for _w, _h, _d, _lv in ((250, 16, 48, 1), (16, 250, 48, 1), (96, 64, 16, 1), (48, 32, 256, 1), (48, 32, 256, MULTI), (33, 47, 64, 1),
                        (17, 16, 32, 1), (16, 16, 256, 1), (16, 16, 16, 1), (16, 16, 16, MULTI), (8, 8, 32, MULTI), (8, 8, 16, 1),
                        (5, 3, 32, 1), (1, 1, 16, 1)):             # largest first
    DOMAIN[f"{_w}x{_h}-d{_d}{'m' if _lv > 1 else ''}"] = (_w, _h, _d, _lv, {}, 7)
SHARP = ("S-aggx16", "S-aggx64", "P-aggx16")                        # peak probability > 0.9, zero pixels in the truth
FLAT = ("S-agg/16", "S-zero")                                       # peak probability < 0.2
ACT4 = ("S-act4", "Sm-act4")                                        # peak probability > 0.75 over 6 planes
ACT4_DEEP = ("P-act4",)                                             # ... > 0.6 over 16 planes (measured 0.70; 16 planes share the mass)
CLAMPED = ("S-aggx16", "S-aggx64", "S-step")                        # the final relu clamps pixels of the truth
D16 = tuple(n for n, g in DOMAIN.items() if g[2] == 16)
_domain_cache = {}


def domain_input(w, h, d, kind):
    """int8 (6, h, w): a seed of synth.model_input_i8, or one of the patterns that reach the int8 limits"""
    if isinstance(kind, int):
        return synth.model_input_i8(w, h, d, kind)
    x = np.empty((6, h, w), np.int8)
    if kind in ("max", "min", "zero"):
        x[:] = {"max": 127, "min": -128, "zero": 0}[kind]
    elif kind == "noise":
        x[:] = np.random.default_rng(1).integers(-128, 128, (6, h, w), dtype=np.int8)
    elif kind == "checker":                                         # pixel frequency, the same in all six planes
        x[:] = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0, 127, -128)
    elif kind == "step":
        x[:, :, :w // 2] = 127
        x[:, :, w // 2:] = -128
    else:
        raise ValueError(kind)
    return x


def domain_blob(levels, wk):
    blob = weights.synthetic(0, levels, head_gain=wk.get("head_gain", 1.0), act_scale=wk.get("act_scale", 1.0))
    return scaled(blob, "agg.out", wk["agg_out"], levels) if "agg_out" in wk else blob


def domain_point(oracle, name):
    """-> (blob, x, x_other, Refs) of a grid point, computed once per process.  x_other is the second input of the liveness
    check: uniform int8 noise of another seed than the grid's noise input (the two eyes differ at every size, so the matching
    costs move even at 1x1, where the texture generator saturates both eyes to the same byte)."""
    if name not in _domain_cache:
        w, h, d, levels, wk, kind = DOMAIN[name]
        blob, x = domain_blob(levels, wk), domain_input(w, h, d, kind)
        x_other = np.random.default_rng(2).integers(-128, 128, (6, h, w), dtype=np.int8)
        _domain_cache[name] = (blob, x, x_other, Refs(oracle, blob, x, d))
    return _domain_cache[name]


def small_failures(stage, a, truth):
    """A stage or map of fewer than MIN_STAGE_VALUES values: every element against the truth under the absolute bounds of
    tests/test_gpu_parity.py — disp_low max < 1e-4, cost max < 2e-4 max(1, max |cost|), a map in pixels (the final one and,
    in their own pixels, the coarse level maps) mean < X3_TOL and max < 20 BUDGET.  Feature maps have 32 channels: never
    fewer than 32 values."""
    e, m, _ = err(a, truth)
    bad = []
    if not np.isfinite(np.asarray(a)).all():
        bad.append("not finite")
    if stage == "disp_low":
        if not m < 1e-4:
            bad.append(f"max {m:.3e} >= 1e-4")
    elif stage == "cost":
        lim = 2e-4 * max(1.0, float(np.abs(truth).max()))
        if not m < lim:
            bad.append(f"max {m:.3e} >= {lim:.3e}")
    elif stage == "disp" or stage.startswith("level"):
        if not e < X3_TOL:
            bad.append(f"mean {e:.3e} >= X3_TOL")
        if not m < 20 * BUDGET:
            bad.append(f"max {m:.3e} >= 20 x BUDGET")
    else:
        raise ValueError(f"{stage}: no absolute bound for a stage of {np.size(truth)} values")
    return bad


def class_failures(r, out, factor, x3=False, stages=None):
    """What a result that claims to be fp32-class misses at one grid point: `out` maps "disp" and the stage names of
    sn_dbg_read (disp_low, cost, feat_l, feat_r, level1..) to arrays.  Stages and maps of at least MIN_STAGE_VALUES values:
    stage_failures / fp32_class_failures with `factor` (and E < X3_TOL with x3); smaller ones: small_failures.
    -> list of "stage: condition missed".  One function for the CPU teeth and for any HIP mode judged on the grid."""
    bad = []
    for s in (stages if stages is not None else out):
        t = r.truth["disp"] if s == "disp" else r.stage_truth(s)
        a = np.asarray(out[s]).reshape(t.shape)
        if t.size < MIN_STAGE_VALUES:
            msgs = small_failures(s, a, t)
        elif s == "disp":
            msgs = fp32_class_failures(a, t, r.E_ref, r.M_ref, factor)
            if x3 and not err(a, t)[0] < X3_TOL:
                msgs.append(f"E {err(a, t)[0]:.3e} >= X3_TOL")
        else:
            msgs = stage_failures(a, t, r.stage_ref(s), factor)
        bad += [f"{s}: {m}" for m in msgs]
    return bad


def forward_as_stages(res):
    """torch_ref.forward's dict under the names class_failures expects"""
    out = {"disp": res["disp"], "disp_low": res["disp_low"], "cost": res["cost"], "feat_l": res["fl"], "feat_r": res["fr"]}
    out.update({f"level{k}": m for k, m in level_maps(res).items()})
    return out


# ---- one engine run (GPU) --------------------------------------------------------------------------------------------------
STAGES_SINGLE = ("disp_low", "cost", "feat_l", "feat_r")   # what a mode keeps in memory after a single-pair call


def read_stages(eng, levels):
    names = STAGES_SINGLE + tuple(f"level{k}" for k in range(1, levels))
    return {s: eng.dbg_read(s).copy() for s in names}


def run_engine(path, prec, x, x_other, levels):
    """fresh handle, one single-pair call on x (the engine keeps `cost` only then), its stages; then a call on another
    input and the stages again — a stage that the second input does not change is not a live readout"""
    from hobot_stereonet_amd import api
    with api.StereoNetHIP(path, precision=prec) as eng:
        disp, raw, returned = infer_flagged(eng, x)
        st = eng.refine_stats()
        st["returned"] = returned
        stages = read_stages(eng, levels)
        infer_flagged(eng, x_other)
        again = read_stages(eng, levels)
    live = {s: not np.array_equal(stages[s], again[s]) for s in stages}
    return disp, raw, st, stages, live


def infer_flagged(eng, x):
    """eng.infer(x) -> (disp, raw, "SN_OK"), or the maps a call that returned SN_ERR_RANGE wrote and "SN_ERR_RANGE" (the
    st["returned"] of run_engine: the activation-range tests judge what such a call handed over)"""
    from hobot_stereonet_amd import api
    try:
        return (*eng.infer(x), "SN_OK")
    except api.StereoNetRangeError as e:
        return (*e.outputs, "SN_ERR_RANGE")


# ---- call sequences on ONE handle (tests/test_auto_sequences.py, tests/test_gpu_auto_sequences.py) ---------------------------
# The frames a stream of calls is made of, at SHAPE_S: name -> the `kind` of domain_input (the three textures are seeds of
# synth.model_input_i8).  Two seed-0 models, one per shape class of sn_auto_envelope_px, at the head gain at which the
# committed call list makes the default precision switch, re-enter and switch again (SEQ_GAIN: chosen from {2, 4, 8} after
# one run that printed limit_px, profiles/auto_sequences.txt).  What "calm" and "hard" mean is a premise that
# tests/test_auto_sequences.py asserts on the truth's own residual, per model.
SEQ_KINDS = {"zero": "zero", "tex4": 4, "tex5": 5, "tex6": 6, "noise": "noise", "checker": "checker", "max": "max", "step": "step",
             "min": "min"}
SEQ_LEVELS = {"single": 1, "multi": MULTI}
SEQ_GAIN = {"single": 2.0, "multi": 2.0}
SEQ_CALM = ("zero", "tex4", "tex5", "tex6")
SEQ_HARD = ("max", "step", "min")
# (a) calm x2, hard, hard, calm x9, hard, calm, noise, hard.  The first self-check sees `zero`, the frame with the smallest
# residual; the ninth calm call is the first one after the re-entry and carries the second self-check, on another frame.
SEQ_CALLS = ("zero", "tex4", "max", "step",
             "tex5", "tex6", "zero", "tex4", "tex5", "tex6", "zero", "tex4", "tex5",
             "min", "tex6", "noise", "max")
# (b) one list, started at `zero`, at a texture and at `min`: whatever frame calibrates the handle, the hard frame with the
# smallest residual (`min` or `step`, the one a widened limit lets through first) is the next but one at the latest
SEQ_ROTATED = ("zero", "min", "tex4", "step", "checker", "max")
SEQ_ROTATIONS = ("zero", "tex4", "min")
_seq_cache = {}


def seq_blob(model):
    return weights.synthetic(0, SEQ_LEVELS[model], head_gain=SEQ_GAIN[model])


def seq_input(frame):
    return domain_input(*SHAPE_S, SEQ_KINDS[frame])


def truth_residual(moved, h, w):
    """`moved` of torch_ref.truth (D_k r_k before the relu, coarsest level first) -> (level_px[k] for k = 0 .., residual_px) as
    sn_get_refine_stats defines them: level 0 over the h x w output map, a coarse level over its whole padded map, and
    residual_px = sum_k 2^k level_px[k]"""
    lv = [float(np.abs(m[:h, :w] if k == 0 else m).mean()) for k, m in enumerate(moved[::-1])]
    return lv, float(sum(v * 2 ** k for k, v in enumerate(lv)))


def seq_point(model, frame):
    """-> (x, truth, level_px, residual_px) of a frame under a model, the truth computed once per process"""
    key = (model, frame)
    if key not in _seq_cache:
        w, h, d = SHAPE_S
        x, moved = seq_input(frame), []
        t = torch_ref.truth(seq_blob(model), x, d, moved)
        _seq_cache[key] = (x, t, *truth_residual(moved, h, w))
    return _seq_cache[key]


AUTO_FIELDS = ("residual_px", "precision_last", "reruns", "switches", "selfcheck_epe_px", "selfcheck_residual_px")


def replay(stats_per_call, levels=1, pure=None):
    """What a handle of the default precision reported after each of its calls (dicts of sn_get_refine_stats with at least
    AUTO_FIELDS, in call order, from the first call of the handle on) against the pure state machine sn_auto_init /
    sn_auto_observe / sn_auto_limit_px: -> [(call index, what the handle did that the state machine would not have done)].

    The model of a blocking call (run_forward, include/stereonet_hip.h): it runs in the mode the state is in; a call that
    runs in F16 on a handle that has had no self-check since it last entered F16 carries one (epe_per_px = selfcheck_epe_px /
    selfcheck_residual_px from then on); the call's residual is observed; a call that ran in F16 and is answered with F16X3
    is repeated, so its map (precision_last) is F16X3's and reruns grows by one.
    Optional keys of a record: "observed_px" — the residual the state machine saw where that is not the one reported (a
    repeated call reports the repeat's residual; its first run's is what was observed); "pairs" (default 1: the self-check
    pair is then the whole call, and selfcheck_residual_px must be the observed residual); "running_px", "limit_px",
    "precision_selected" — compared when present.  A call whose range check fired (SN_ERR_RANGE) reports residual_px = +inf:
    it is observed like any other (the state machine leaves F16 at once), owes no self-check and never re-enters F16.
    `pure`: the library (default api.load_library())."""
    import ctypes as C
    from hobot_stereonet_amd import api
    lib = pure or api.load_library()
    s = api.SnAutoState()
    assert lib.sn_auto_init(C.byref(s), levels) == 0
    calibrated, reruns, check = False, 0, (-1.0, -1.0)
    bad = []
    for i, r in enumerate(stats_per_call):
        seen = r.get("observed_px", r["residual_px"])
        start = s.mode
        got_check = (r["selfcheck_epe_px"], r["selfcheck_residual_px"])
        if start == api.PREC_F16 and not calibrated and np.isinf(seen):
            # a call the range check flagged (residual +inf) owes no self-check: there is nothing to calibrate on
            if got_check != check:
                bad.append((i, f"self-check values changed ({check} -> {got_check}) on a call whose range check fired"))
        elif start == api.PREC_F16 and not calibrated:
            entered = s.switches > 0
            if not (got_check[0] >= 0 and got_check[1] >= 0) or (r.get("pairs", 1) == 1 and abs(got_check[1] - seen) > 1e-9):
                bad.append((i, ("re-entry to F16 without a new self-check" if entered else "first F16 call without a self-check")
                            + f": self-check residual {got_check[1]!r}, this call's {seen!r}"))
            s.epe_per_px = got_check[0] / got_check[1] if got_check[1] > 1e-6 else 0.0
            calibrated = True
        elif got_check != check:
            bad.append((i, f"self-check values changed ({check} -> {got_check}) in a call that owes none"))
        check = got_check
        limit, calm = lib.sn_auto_limit_px(C.byref(s)), s.calm
        after = lib.sn_auto_observe(C.byref(s), seen)
        if start == api.PREC_F16X3 and after == api.PREC_F16:
            calibrated = False
        repeat = start == api.PREC_F16 and after == api.PREC_F16X3
        reruns += int(repeat)
        want_last = api.PREC_NAMES[api.PREC_F16X3 if repeat else start]
        if r["precision_last"] != want_last:
            if repeat:
                bad.append((i, f"map returned in {r['precision_last']} although residual {seen:.4f} > limit {limit:.4f} demanded the repeat"))
            elif start == api.PREC_F16X3:
                bad.append((i, f"map returned in {r['precision_last']}: re-entry after {calm} calm calls, "
                               f"the state machine is in f16x3 (residual {seen:.4f}, limit {limit:.4f})"))
            else:
                bad.append((i, f"map returned in {r['precision_last']}, the state machine ran f16 (residual {seen:.4f}, limit {limit:.4f})"))
        if r["switches"] != s.switches:
            bad.append((i, f"{'extra' if r['switches'] > s.switches else 'missing'} switch: handle {r['switches']}, state machine "
                           f"{s.switches} (residual {seen:.4f}, limit {limit:.4f})"))
        if r["reruns"] != reruns:
            bad.append((i, f"reruns {r['reruns']}, state machine {reruns}"))
        if "precision_selected" in r and r["precision_selected"] != api.PREC_NAMES[s.mode]:
            bad.append((i, f"precision_selected {r['precision_selected']}, state machine {api.PREC_NAMES[s.mode]}"))
        if "running_px" in r and abs(r["running_px"] - s.running_px) > 1e-9:
            bad.append((i, f"running_px {r['running_px']!r}, state machine {s.running_px!r}"))
        if "limit_px" in r and abs(r["limit_px"] - lib.sn_auto_limit_px(C.byref(s))) > 1e-9:
            bad.append((i, f"limit_px {r['limit_px']!r}, state machine {lib.sn_auto_limit_px(C.byref(s))!r}"))
    return bad


def trajectory_is_live(stats_per_call):
    """-> (switch with a repeat, re-entry to f16 after it, second switch after that) as call indices, None where missing"""
    up = back = again = None
    prev = {"switches": 0, "reruns": 0, "precision_last": "f16"}
    for i, r in enumerate(stats_per_call):
        rose = r["switches"] > prev["switches"]
        if up is None and rose and r["reruns"] > prev["reruns"] and r["precision_last"] == "f16x3":
            up = i
        elif up is not None and back is None and r["precision_last"] == "f16":
            back = i
        elif back is not None and again is None and rose and r["precision_last"] == "f16x3":
            again = i
        prev = r
    return up, back, again


# ---- the activation range (tests/test_truth64_range.py, tests/test_gpu_truth64_range.py) -------------------------------------
# The network is positively homogeneous between its first layer and its head (leaky relu, zero padding, residual adds and the
# cost volume's difference all commute with a positive scale), so scaling the first layer and every bias after it by s and the
# head's weights by 1/s leaves the function unchanged — with s = 2^k bit for bit, in float64 and in fp32 alike.  One truth and
# one Refs judge every point of the axis; what changes is where the values the fp16 modes STORE between two layers sit in the
# fp16 format.
F16_MAX = 65504.0            # the largest finite fp16
F16_MIN_NORMAL = 2.0 ** -14
SUB_CAP = 0.05               # in range: at most this share of a tensor's non-zero values below F16_MIN_NORMAL (a cap on the input)


def _scale(out, table, name, gain):
    off, shape = table[name]
    out[off:off + int(np.prod(shape))] *= np.float32(gain)


def gauge(blob, levels, tower=1.0, low=1.0, only_level=None):
    """-> a copy of `blob` that computes the same function with its stored activations scaled: the refinement towers' by
    `tower` (every level, or `only_level` alone), the low-resolution branch's by `low`.  Powers of two are exact."""
    out, table = blob.copy(), spec.offsets(levels)
    if tower != 1.0:
        for lv in (range(levels) if only_level is None else [only_level]):
            p = spec.ref_prefix(lv)
            _scale(out, table, p + ".in.w", tower)
            _scale(out, table, p + ".in.b", tower)
            for i in range(spec.N_REF_RES):
                for j in (1, 2):
                    _scale(out, table, f"{p}.res{i}.{j}.b", tower)
            _scale(out, table, p + ".out.w", 1.0 / tower)
    if low != 1.0:
        _scale(out, table, "feat.down0.w", low)
        _scale(out, table, "feat.down0.b", low)
        names = [f"feat.down{i}" for i in range(1, spec.N_DOWN)] + [f"feat.res{i}.{j}" for i in range(spec.N_FEAT_RES) for j in (1, 2)]
        for n in names + ["feat.out"] + [f"agg.conv{i}" for i in range(spec.N_AGG)]:
            _scale(out, table, n + ".b", low)
        _scale(out, table, "agg.out.w", 1.0 / low)
    return out


def range_profile(blob, x, d):
    """The float64 truth of (blob, x) with every 32-channel tensor of it looked at on the way: the outputs of torch_ref's
    convolutions and leaky relus, its residual sums and its cost volume (the head outputs and the cost are fp32 in every
    mode of the engine: not counted).  -> (truth, profile); profile["tower"], profile["low"] and profile["levels"][k] (the
    tower of refinement level k) are (A_max, sub): the largest |v|, and the largest per-tensor share of non-zero values
    below 2^-14."""
    import contextlib
    import torch
    stats, where = {}, ["low"]

    def see(t):
        if t.dim() >= 4 and t.shape[1] == spec.C:
            a = t.detach().abs()
            nz = a > 0
            n = int(nz.sum())
            share = float(((a < F16_MIN_NORMAL) & nz).sum()) / n if n else 0.0
            for key in where:
                m, s = stats.get(key, (0.0, 0.0))
                stats[key] = (max(m, float(a.max())), max(s, share))
        return t

    orig = {"conv2d": torch_ref.F.conv2d, "conv3d": torch_ref.F.conv3d, "lrelu": torch_ref.lrelu, "cost_volume": torch_ref.cost_volume,
            "res_block": torch_ref.res_block, "refine": torch_ref.refine}

    def res_block(blob_, prefix, t, dil):               # torch_ref.res_block with its residual sum in view
        dt = t.dtype
        u = torch_ref.lrelu(torch_ref.F.conv2d(t, torch_ref._t(blob_, prefix + ".1.w", dt), torch_ref._t(blob_, prefix + ".1.b", dt),
                                               padding=dil, dilation=dil))
        u = torch_ref.F.conv2d(u, torch_ref._t(blob_, prefix + ".2.w", dt), torch_ref._t(blob_, prefix + ".2.b", dt), padding=dil,
                               dilation=dil)
        return torch_ref.lrelu(see(t + u))

    def refine(blob_, disp_up, img, dmax, prefix="ref", moved=None):
        level = 0 if prefix == "ref" else int(prefix[3:])
        where[:] = ["tower", ("levels", level)]
        try:
            return orig["refine"](blob_, disp_up, img, dmax, prefix, moved)
        finally:
            where[:] = ["low"]

    @contextlib.contextmanager
    def hooked():
        torch_ref.F.conv2d = lambda *a, **k: see(orig["conv2d"](*a, **k))
        torch_ref.F.conv3d = lambda *a, **k: see(orig["conv3d"](*a, **k))
        torch_ref.lrelu = lambda t: see(orig["lrelu"](t))
        torch_ref.cost_volume = lambda *a: see(orig["cost_volume"](*a))
        torch_ref.res_block, torch_ref.refine = res_block, refine
        try:
            yield
        finally:
            torch_ref.F.conv2d, torch_ref.F.conv3d = orig["conv2d"], orig["conv3d"]
            for k in ("lrelu", "cost_volume", "res_block", "refine"):
                setattr(torch_ref, k, orig[k])
    with hooked():
        t = torch_ref.truth(blob, x, d)
    prof = {"tower": stats["tower"], "low": stats["low"], "levels": {k[1]: v for k, v in stats.items() if isinstance(k, tuple)}}
    return t, prof


def range_class(a_max, sub):
    """One branch's (A_max, sub) against the fp16 format alone -> "in range" (one binade of margin below 65504: the fp16
    paths' stored values differ from the truth's by parts in a thousand, never by a factor of two; at most SUB_CAP of a
    tensor below the normal range), "overflows" (one binade above), or "guard band" (anything between)"""
    if a_max <= F16_MAX / 2 and sub <= SUB_CAP:
        return "in range"
    if a_max >= 2 * F16_MAX:
        return "overflows"
    return "guard band"


def point_class(prof):
    """-> the class of a grid point: overflows if a branch does, in range if both are, else guard band"""
    c = {range_class(*prof["tower"]), range_class(*prof["low"])}
    return "overflows" if "overflows" in c else ("in range" if c == {"in range"} else "guard band")


# name: (levels, k_tower, k_low, only_level); all at SHAPE_S, weights seed 0, input seed 4.  "top" points sit at the largest k
# of an axis that is in range (tests/test_truth64_range.py computes that they do).  The tower peaks at 6.2 where the
# low-resolution branch peaks at 10.8, so 2^14 takes the low branch past 2 x 65504 and leaves the tower (1.0e5) in the guard
# band, and 2^13 leaves both there: the tower axes carry k = 15 and the low axis k = 14 as well, so that every axis has two
# points that overflow by the rule of range_class.
RANGE_INPUT = 4
RANGE_TOWER_K = (-8, -4, 4, 8, 12, 13, 14, 15, 16)
RANGE_LOW_K = (-8, -4, 4, 8, 11, 12, 13, 14, 16)
RANGE_TOWER_K_MULTI = (-4, 8, 12, 14, 15, 16)
RANGE_LOW_K_MULTI = (-4, 8, 11, 14, 16)
RANGE_TOP = {"tower": 12, "low": 11}
RANGE = {"S-k0": (1, 0, 0, None), "M-k0": (MULTI, 0, 0, None)}
for _k in RANGE_TOWER_K:
    RANGE[f"S-tower{_k:+d}"] = (1, _k, 0, None)
for _k in RANGE_LOW_K:
    RANGE[f"S-low{_k:+d}"] = (1, 0, _k, None)
RANGE["S-both-top"] = (1, RANGE_TOP["tower"], RANGE_TOP["low"], None)
for _k in RANGE_TOWER_K_MULTI:
    RANGE[f"M-tower{_k:+d}"] = (MULTI, _k, 0, None)
for _k in RANGE_LOW_K_MULTI:
    RANGE[f"M-low{_k:+d}"] = (MULTI, 0, _k, None)
RANGE["M-level2+14"] = (MULTI, 14, 0, 2)       # one coarse tower alone: 4.8e4, guard band
RANGE["M-level2+16"] = (MULTI, 16, 0, 2)       # ... and past the end of the format
RANGE_BASE = {1: "S-k0", MULTI: "M-k0"}
_range_cache, _range_refs = {}, {}


def range_blob(name):
    levels, kt, kl, only = RANGE[name]
    return gauge(weights.synthetic(0, levels), levels, 2.0 ** kt, 2.0 ** kl, only)


def range_point(name):
    """-> (blob, truth, profile) of a grid point, computed once per process"""
    if name not in _range_cache:
        blob = range_blob(name)
        _range_cache[name] = (blob, *range_profile(blob, domain_input(*SHAPE_S, RANGE_INPUT), SHAPE_S[2]))
    return _range_cache[name]


def range_refs(oracle, levels):
    """ONE Refs per model, from the k = 0 blob: the truth and both fp32 checkers are bit-identical along the gauge
    (tests/test_truth64_range.py), so it judges every point.  -> (x, x_other, Refs)"""
    if levels not in _range_refs:
        x = domain_input(*SHAPE_S, RANGE_INPUT)
        x_other = np.random.default_rng(2).integers(-128, 128, x.shape, dtype=np.int8)
        _range_refs[levels] = (x, x_other, Refs(oracle, range_blob(RANGE_BASE[levels]), x, SHAPE_S[2]))
    return _range_refs[levels]
