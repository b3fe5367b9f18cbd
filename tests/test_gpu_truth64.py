"""Every precision mode of the HIP path against the float64 truth (tests/golden/torch_ref.truth), not against the fp32
oracle: the oracle is itself 6-8e-5 px (mean) and up to 0.8e-3 px (one pixel) from the truth at 1280x720
(tests/test_truth64.py), the size of what used to be reported for the two "exact" modes.  HIP path through the C ABI
(the network behind DnnNode::Run, stereonet_infer/src/stereonet_node.cpp:812).  Needs an MI355X.

    E(a) = mean |a - truth|, M(a) = max |a - truth|, S(a) = mean (a - truth);
    E_ref = max(E(oracle), E(torch fp32)), M_ref likewise — computed live from the two CPU fp32 implementations on the
    same input, never from a HIP result.  No pixel is left out of any comparison.

1. the budget: E < 1e-3 for FP32, F16X3 and the default precision everywhere, for forced F16 at head gain 1; at head gain 8
   forced F16 is over it and the default ran f16x3;
2. fp32-class: FP32 within 3 x (E_ref, M_ref) — a third fp32 summation order, not a lost bit; F16X3 within 4 x (22-bit
   operands: unit round-off 4 x fp32's) and E < 2e-4;
3. stage by stage (sn_dbg_read after a single-pair call, shown live by a second input): disp_low within 3 x (FP32) / 4 x
   (fp16 modes: the low-resolution branch is 22-bit split in both) of the CPU checkers' own error at that stage, cost and
   features likewise against the fp32 torch run's, the coarse level maps of the hierarchical model likewise where the
   towers are fp32-class (FP32, F16X3) and below 1e-3 / 2^k px where level k ran on the fp16 tower at head gain 1 (its
   error reaches the final map doubled k times); F16 and F16X3 share the low-resolution branch bit for bit;
4. bias: |S| <= E_ref for FP32 and F16X3 (round-off is not coherent, a lost operand bit is); the sum-preserving weight
   rounding of F16 halves |S| of SN_W_ROUND=rne against the truth too;
5. finite, raw >= 0, raw == rint(disp * inv_q).
Every tolerance is 1e-3 / 2e-4 (the project's own) or a 3 x / 4 x / 1 x factor over the live E_ref / M_ref.
Measured (profiles/r08_truth64.txt): FP32 0.85-1.03 x E_ref, F16X3 0.32-0.45 x E_ref, |S| <= 0.11 x E_ref in both."""
import time

import numpy as np
import pytest

from hobot_stereonet_amd import api, spec, synth, weights

pytestmark = pytest.mark.gpu

SHAPES = {"C1": (960, 540, 48, 1), "C2": (1280, 720, 192, 1), "C5m": (1242, 375, 256, spec.MULTI_LEVELS),
          "pad": (124, 38, 32, 1)}            # pad: not a multiple of 16 on either axis
# (shape, weight seed, head gain, input seed): seed 0 everywhere; at C2 / C5 the worst draws tests/test_gpu_seeds.py names
GRID = [("pad", 0, 1.0, 22), ("C1", 0, 1.0, 21), ("C2", 0, 1.0, 0), ("C5m", 0, 1.0, 22),
        ("C2", 6, 1.0, 506), ("C2", 7, 1.0, 507), ("C2", 1, 8.0, 501),
        ("C5m", 3, 1.0, 503), ("C5m", 7, 1.0, 507), ("C5m", 1, 8.0, 501)]
MODES = [("fp32", api.PREC_FP32), ("f16x3", api.PREC_F16X3), ("f16", api.PREC_F16), ("auto", api.PREC_DEFAULT)]
_cache = {}
_t_refs = [0.0]


def _id(g):
    return f"{g[0]}-w{g[1]}-g{g[2]:g}-in{g[3]}"


def _refs(oracle, g):
    """module-wide cache: the float64 truth, the oracle and the fp32 torch run of a grid point are computed once"""
    import truth_compare as tc
    if g not in _cache:
        shape, ws, gain, si = g
        w, h, d, levels = SHAPES[shape]
        t0 = time.time()
        blob = weights.synthetic(ws, levels, head_gain=gain)
        x = synth.model_input_i8(w, h, d, si)
        _cache[g] = (blob, x, synth.model_input_i8(w, h, d, si + 1000), tc.Refs(oracle, blob, x, d))
        _t_refs[0] += time.time() - t0
    return _cache[g]


def _model(tmp_path, blob, w, h, d):
    p = str(tmp_path / "m.snw")
    weights.save_snw(p, blob, w, h, d)
    return p


def _run(path, prec, x, x_other, levels):
    """truth_compare.run_engine (shared with tests/test_gpu_truth64_domain.py): fresh handle, one single-pair call, the
    stages, and whether a second input changes each readout"""
    import truth_compare as tc
    return tc.run_engine(path, prec, x, x_other, levels)


@pytest.mark.parametrize("g", GRID, ids=_id)
def test_modes_against_the_truth(oracle, tmp_path, g):
    import truth_compare as tc
    shape, ws, gain, si = g
    w, h, d, levels = SHAPES[shape]
    blob, x, x_other, r = _refs(oracle, g)
    path = _model(tmp_path, blob, w, h, d)
    truth = r.truth["disp"]
    inv_q = np.float32(1.0 / (192.0 * float(np.float32(spec.OUT_SCALE))))
    print(f"\n== {_id(g)}  {w}x{h} D={d} levels={levels}: E_ref {r.E_ref:.2e} M_ref {r.M_ref:.2e}; oracle E/M/S {tc.fmt(r.e_oracle['disp'])}, "
          f"torch fp32 {tc.fmt(r.e_t32['disp'])}; zero pixels in the truth {int((truth == 0).sum())}")
    print("   stage refs (E/M of the CPU fp32 checkers): " + "  ".join(f"{k} {tc.fmt(v)}" for k, v in r.ref.items() if k != "disp"))
    bad, low_of = [], {}
    for mname, prec in MODES:
        disp, raw, st, stages, live = _run(path, prec, x, x_other, levels)
        e = tc.err(disp, truth)
        ran = st["precision_last"]
        row = f"   {mname:<6} ran {ran:<6} E/M/S {tc.fmt(e)}"
        fail = lambda msg: bad.append(f"{mname}: {msg}")
        # 5. the wire
        if not (np.isfinite(disp).all() and raw.min() >= 0 and (raw == np.rint(disp * inv_q).astype(np.int32)).all()):
            fail("output not finite, negative, or raw != rint(disp * inv_q)")
        # 1. the budget
        if mname == "f16" and gain > 1.0:
            if not e[0] > tc.BUDGET:
                fail(f"forced F16 at head gain {gain:g} is inside the budget ({e[0]:.3e}): the grid point does not test AUTO")
        elif not e[0] < tc.BUDGET:
            fail(f"E {e[0]:.3e} >= {tc.BUDGET:g}")
        if mname == "auto" and gain > 1.0 and ran != "f16x3":
            fail(f"default precision ran {ran} at head gain {gain:g}")
        if mname != "auto" and ran != mname:
            fail(f"forced mode ran {ran}")
        # 2. + 4. fp32-class
        if mname == "fp32":
            for m in tc.fp32_class_failures(disp, truth, r.E_ref, r.M_ref, tc.FP32_FACTOR):
                fail(m)
        if mname == "f16x3":
            for m in tc.fp32_class_failures(disp, truth, r.E_ref, r.M_ref, tc.X3_FACTOR):
                fail(m)
            if not e[0] < tc.X3_TOL:
                fail(f"E {e[0]:.3e} >= X3_TOL")
        # 3. stage by stage
        factor = tc.FP32_FACTOR if mname == "fp32" else tc.X3_FACTOR
        for s, a in stages.items():
            if not live[s]:
                row += f" | {s} NOT LIVE"
                fail(f"{s}: a second input does not change the readout")
                continue
            t = r.stage_truth(s)
            es = tc.err(a.reshape(t.shape), t)
            row += f" | {s} {tc.fmt(es[:2])}"
            if s.startswith("level") and ran == "f16":
                # a coarse map of the fp16 tower (11-bit operands: the 4 x factor of split operands does not apply to it).
                # Level k works in 1/2^k-resolution pixels and every finer level doubles the values it passes on, so an
                # error e_k arrives in the final map as 2^k e_k: inside the budget it must itself be below 1e-3 / 2^k.
                k = int(s[5:])
                if not np.isfinite(a).all():
                    fail(f"{s}: not finite")
                if gain == 1.0 and not es[0] < tc.BUDGET / 2 ** k:
                    fail(f"{s}: mean {es[0]:.3e} >= {tc.BUDGET:g} / 2^{k}")
                continue
            for m in tc.stage_failures(a.reshape(t.shape), t, r.stage_ref(s), factor):
                fail(f"{s}: {m}")
        low_of[mname] = stages["disp_low"]
        print(row)
    if not np.array_equal(low_of["f16"], low_of["f16x3"]):
        bad.append("disp_low of F16 and F16X3 differ: the low-resolution branch takes no mode")
    print(f"   CPU references so far {_t_refs[0]:.0f} s ({len(_cache)} truths)")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("g", [("C2", 6, 1.0, 506), ("C5m", 3, 1.0, 503)], ids=_id)
def test_sum_preserving_rounding_halves_the_bias_against_the_truth(oracle, tmp_path, monkeypatch, g):
    """tests/test_gpu_seeds.py's A/B of the fp16 tower's weight rounding on the two worst draws, against the truth: the
    coherent offset round-to-nearest fp16 weights add up to is what the sum-preserving rounding takes out."""
    import truth_compare as tc
    shape, ws, gain, si = g
    w, h, d, levels = SHAPES[shape]
    blob, x, _, r = _refs(oracle, g)
    path = _model(tmp_path, blob, w, h, d)
    res = {}
    for mode in ("rne", "sum"):
        if mode == "rne":
            monkeypatch.setenv("SN_W_ROUND", "rne")
        else:
            monkeypatch.delenv("SN_W_ROUND", raising=False)
        with api.StereoNetHIP(path, precision=api.PREC_F16) as eng:
            disp, _ = eng.infer(x)
        res[mode] = tc.err(disp, r.truth["disp"])
    print(f"\n== {_id(g)} F16 weight rounding, E/M/S vs truth: rne {tc.fmt(res['rne'])}, sum-preserving {tc.fmt(res['sum'])}; "
          f"oracle's own {tc.fmt(r.e_oracle['disp'])}")
    assert res["sum"][0] < tc.BUDGET
    assert abs(res["sum"][2]) < 0.5 * abs(res["rne"][2])
