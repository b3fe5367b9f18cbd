"""Every precision mode of the HIP path against the float64 truth ACROSS THE INPUT DOMAIN: tests/test_gpu_truth64.py's
mode loop and criteria (truth_compare, nothing new) at small shapes over the grid truth_compare.DOMAIN, whose premises
tests/test_truth64_domain.py checks on the CPU — a soft-argmin from flat (peak probability 0.18) to near one-hot (0.99),
images at the int8 limits (saturated, textureless, pixel-frequency checkerboard, a hard step, plain noise), a final relu
that clamps up to all pixels, and the geometries sn_create accepts but nothing ran: D = 16 (one cost plane), 1x1 low-resolution
maps, W or H below 16, wl < Dl.  Needs an MI355X.

Per grid point, per mode (fresh handle, one single-pair call, then a second input for the liveness of every readout):
a. wire: finite, raw >= 0, raw == rint(disp * inv_q);
b. known answers: D = 16 gives disp_low of all zero bits; F16 and F16X3 share disp_low, cost and both feature maps bit for
   bit; every stage read is live (not demanded where the truth of the stage is the same for both inputs: disp_low at D = 16);
c. FP32 and F16X3: truth_compare.class_failures — stages and maps of >= MIN_STAGE_VALUES values within 3 x / 4 x the CPU
   checkers' own error at that stage (F16X3 also E < 2e-4), smaller ones element by element under the absolute bounds of
   tests/test_gpu_parity.py;
d. forced F16: finite, E recorded — no budget is claimed for it outside the base regime;
e. the default precision (the product claim): E < 1e-3 in the first call of a fresh handle, its map bit-identical to the
   forced mode refine_stats()["precision_last"] names, and f16x3 wherever forced F16 measured E >= 1e-3;
f. hierarchical points: coarse level maps fp32-class where the tower is (c), below 1e-3 / 2^k where level k ran on the fp16
   tower at head gain 1 with the default act_scale.
Every bound is BUDGET, X3_TOL, FP32_FACTOR, X3_FACTOR or a parity bound; every live one comes from the CPU references.
Measured (profiles/truth64_domain.txt): every point passes; FP32 0.53-1.30 x E_ref, F16X3 0.19-1.35 x, the default precision
E <= 5.6e-4 px (f16x3 at the two head-gain-8 points, where forced F16 is at 1.7e-3 / 1.9e-3 px)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import truth_compare as tc
from hobot_stereonet_amd import api, spec, weights

pytestmark = pytest.mark.gpu

MODES = [("fp32", api.PREC_FP32), ("f16x3", api.PREC_F16X3), ("f16", api.PREC_F16), ("auto", api.PREC_DEFAULT)]
INV_Q = np.float32(1.0 / (192.0 * float(np.float32(spec.OUT_SCALE))))


def _model(tmp_path, blob, w, h, d):
    p = str(tmp_path / "m.snw")
    weights.save_snw(p, blob, w, h, d)
    return p


def _wire_ok(disp, raw):
    return bool(np.isfinite(disp).all() and raw.min() >= 0 and (raw == np.rint(disp * INV_Q).astype(np.int32)).all())


@pytest.mark.parametrize("name", list(tc.DOMAIN))
def test_modes_against_the_truth_across_the_domain(oracle, tmp_path, name):
    import torch_ref
    w, h, d, levels, wk, kind = tc.DOMAIN[name]
    blob, x, x_other, r = tc.domain_point(oracle, name)
    path = _model(tmp_path, blob, w, h, d)
    truth = r.truth["disp"]
    peak, zeros = tc.describe(r.truth)
    other = []

    def truth_moves(stage):
        """liveness is decided from the truth: a readout has to change only where the truth of that stage does (one cost
        plane gives disp_low = 0 whatever the input); the second input's truth is computed when a readout stood still"""
        if not other:
            other.append(tc.forward_as_stages(torch_ref.truth(blob, x_other, d)))
        return not np.array_equal(other[0][stage], r.stage_truth(stage))
    base_regime = wk.get("head_gain", 1.0) == 1.0 and wk.get("act_scale", 1.0) == 1.0 and "agg_out" not in wk
    print(f"\n== {name}  {w}x{h} D={d} levels={levels} weights {wk or 'default'} input {kind}: peak probability {peak:.3f}, zero pixels "
          f"{100 * zeros:.1f} %, E_ref {r.E_ref:.2e} M_ref {r.M_ref:.2e}")
    print("   stage refs (E/M of the CPU fp32 checkers): " + "  ".join(f"{k} {tc.fmt(v)}" for k, v in r.ref.items() if k != "disp"))
    bad, got = [], {}
    for mname, prec in MODES:
        disp, raw, st, stages, live = tc.run_engine(path, prec, x, x_other, levels)
        e = tc.err(disp, truth)
        ran = st["precision_last"]
        got[mname] = (disp, stages, e, ran)
        ratio = f"{e[0] / r.E_ref:.2f} x E_ref" if r.E_ref > 0 else "E_ref 0"
        row = f"   {mname:<6} ran {ran:<6} E/M/S {tc.fmt(e)} ({ratio})"
        fail = lambda msg: bad.append(f"{mname}: {msg}")
        for s, a in stages.items():
            t = r.stage_truth(s)
            row += f" | {s} {tc.fmt(tc.err(a.reshape(t.shape), t)[:2])}"
        print(row)
        # a. the wire
        if not _wire_ok(disp, raw):
            fail("output not finite, negative, or raw != rint(disp * inv_q)")
        if mname != "auto" and ran != mname:
            fail(f"forced mode ran {ran}")
        # b. known answers
        if d == 16 and stages["disp_low"].view(np.uint32).any():
            fail("disp_low of a single cost plane is not all zero bits")
        for s in stages:
            if not live[s] and truth_moves(s):
                fail(f"{s}: a second input does not change the readout")
        # c. fp32-class modes (f: their coarse level maps are stages of it)
        if mname in ("fp32", "f16x3"):
            for m in tc.class_failures(r, {"disp": disp, **stages}, tc.FP32_FACTOR if mname == "fp32" else tc.X3_FACTOR, x3=mname == "f16x3"):
                fail(m)
        # d. / f. the fp16 tower
        if ran == "f16":
            for s, a in stages.items():
                if not np.isfinite(a).all():
                    fail(f"{s}: not finite")
                if s.startswith("level") and base_regime:
                    k, t = int(s[5:]), r.stage_truth(s)
                    es = tc.err(a.reshape(t.shape), t)
                    if not es[0] < tc.BUDGET / 2 ** k:
                        fail(f"{s}: mean {es[0]:.3e} >= {tc.BUDGET:g} / 2^{k}")
    # b. the low-resolution branch takes no mode
    for s in tc.STAGES_SINGLE:
        if not np.array_equal(got["f16"][1][s], got["f16x3"][1][s]):
            bad.append(f"{s} of F16 and F16X3 differ: the low-resolution branch takes no mode")
    # e. the default precision
    adisp, _, ae, aran = got["auto"]
    if not ae[0] < tc.BUDGET:
        bad.append(f"auto: E {ae[0]:.3e} >= {tc.BUDGET:g} (ran {aran})")
    if aran not in ("f16", "f16x3"):
        bad.append(f"auto: ran {aran}")
    elif not np.array_equal(adisp, got[aran][0]):
        bad.append(f"auto: ran {aran} but its map is not the forced {aran} map (max difference {np.abs(adisp - got[aran][0]).max():.3e})")
    else:
        bad += [f"auto: ran {aran} but its {s} is not the forced {aran} mode's" for s in tc.STAGES_SINGLE
                if not np.array_equal(got["auto"][1][s], got[aran][1][s])]
    if not got["f16"][2][0] < tc.BUDGET and aran != "f16x3":
        bad.append(f"auto: ran {aran} where forced F16 has E {got['f16'][2][0]:.3e} >= {tc.BUDGET:g}")
    print(f"   default precision ran {aran}; forced F16 {'over' if not got['f16'][2][0] < tc.BUDGET else 'inside'} the budget")
    assert not bad, "\n".join(bad)


# ---- the other kernel pairings of the low-resolution branch at the hard points ------------------------------------------------
PAIRING_POINTS = ("S-aggx64", "P-aggx16", "250x16-d48", "16x250-d48")
PAIRING_ENVS = [{"SN_HEAD_FOLD": "0"},
                {"SN_AGG_DMA": "0", "SN_FEAT_DMA": "0", "SN_DOWN_DMA": "0", "SN_HEAD_FOLD": "0"},
                {"SN_DOWN01": "0"}]
_CHILD = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, os.path.join(root, "tests", "golden")]
import truth_compare as tc
from hobot_stereonet_amd import api, weights
for name in sys.argv[3:]:
    w, h, d, levels, wk, kind = tc.DOMAIN[name]
    path = os.path.join(out, "m.snw")
    weights.save_snw(path, tc.domain_blob(levels, wk), w, h, d)
    with api.StereoNetHIP(path, precision=api.PREC_F16X3) as eng:
        disp, raw = eng.infer(tc.domain_input(w, h, d, kind))
        np.savez(os.path.join(out, name.replace("/", "_") + ".npz"), disp=disp, raw=raw, disp_low=eng.dbg_read("disp_low"),
                 cost=eng.dbg_read("cost"))
"""


def test_other_kernel_pairings_at_the_hard_points(oracle, tmp_path):
    """SN_HEAD_FOLD=0 (k_head_softargmin instead of the folded epilogue + k_softargmin_p), the plain-tensor kernels of the
    whole low-resolution branch, and the unfolded first two down-convs, in SN_PREC_F16X3 at the sharpest soft-argmin and
    the two 1-row / 1-column low-resolution maps: disp_low, cost and the final map judged as in (c).  One child process per
    environment (the switches are read once per process), one after another."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    script = tmp_path / "run.py"
    script.write_text(_CHILD)
    bad = []
    for i, env in enumerate(PAIRING_ENVS):
        out = tmp_path / f"env{i}"
        out.mkdir()
        p = subprocess.run([sys.executable, str(script), root, str(out), *PAIRING_POINTS], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (env, p.stderr[-2000:])            # nothing more is started after a child that failed
        for name in PAIRING_POINTS:
            r = tc.domain_point(oracle, name)[3]
            got = np.load(out / (name.replace("/", "_") + ".npz"))
            res = {s: got[s] for s in ("disp", "disp_low", "cost")}
            if not _wire_ok(got["disp"], got["raw"]):
                bad.append(f"{env} {name}: output not finite, negative, or raw != rint(disp * inv_q)")
            msgs = tc.class_failures(r, res, tc.X3_FACTOR, x3=True)
            rows = [f"{s} {tc.fmt(tc.err(a.reshape(r.stage_truth(s).shape), r.stage_truth(s))[:2])}" for s, a in res.items()]
            print(f"\n{env} {name}: E/M " + "  ".join(rows) + (f"  FAILS: {msgs}" if msgs else ""))
            bad += [f"{env} {name}: {m}" for m in msgs]
    assert not bad, "\n".join(bad)
