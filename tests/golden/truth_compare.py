"""Judging a disparity map (or any stage of the network) against the float64 truth (torch_ref.truth) — shared by
tests/test_truth64.py (what the CPU checkers themselves are worth) and tests/test_gpu_truth64.py (every precision mode
of the HIP path).  Nothing here looks at a HIP result to set a bound: E_ref / M_ref come from the two CPU fp32
implementations (the C oracle and the fp32 torch run) on the same input, and there is no exclusion mask.

    E(a) = mean |a - truth|      M(a) = max |a - truth|      S(a) = mean (a - truth)   (signed: the coherent part)
"""
from __future__ import annotations

import time

import numpy as np

import torch_ref

BUDGET = 1e-3          # px: the project's bound on the mean error of a full-size map (north star; F16_TOL)
X3_TOL = 2e-4          # px: what "fp32-class" has promised for SN_PREC_F16X3 since round 4
FP32_FACTOR = 3.0      # a third fp32 summation order next to the two CPU ones (they differ by 1.4x from each other)
X3_FACTOR = 4.0        # 22-bit split operands: unit round-off 4x that of fp32's 24 bits


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

