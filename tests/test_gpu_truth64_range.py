"""Every precision mode of the HIP path against the float64 truth ALONG THE ACTIVATION RANGE: the grid truth_compare.RANGE, whose
premises tests/test_truth64_range.py checks on the CPU.  A power-of-two gauge moves the values the fp16 modes STORE between two
layers (fp16, or a hi/lo pair of fp16: both end at 65504) from 2^-8 to 2^16 times where the synthetic weights put them, in the
refinement towers, in the low-resolution branch or in one coarse tower alone, and leaves the function — the truth, the fp32 torch
run and the C oracle — bit-identical: ONE Refs per model judges every point.  A point's class (in range / guard band / overflows)
comes from the truth's own activations and the fp16 format (truth_compare.range_class), never from an engine result.  Needs an
MI355X.

Per grid point, per mode (tests/test_gpu_truth64_domain.py's loop: fresh handle, one single-pair call):
a. wire: finite, raw >= 0, raw == rint(disp * inv_q) — every point;
u. the universal rule — every point: a call that returns SN_OK with nothing flagged has a map within its mode's own bound
   (FP32, F16X3: class_failures on the map; F16 and the default precision: E < BUDGET); SN_ERR_RANGE is returned exactly when a
   count of refine_stats() (nonfinite_px, nonfinite_low_px) is non-zero;
p. SN_PREC_FP32 — every point: map and raw bit-identical to the k = 0 map of the same model, never flagged (a power-of-two gauge
   is exact in fp32: a difference is an fp16 step inside the fp32 path);
in range: nothing flagged; criteria c, d, e, f of the domain test unchanged; F16 and F16X3 share disp_low, cost and the feature
   maps bit for bit; max |map_k - map_0| of F16 and F16X3 recorded;
overflows: F16, F16X3 and the default precision (after its repeat) return SN_ERR_RANGE, and the counts name the branch: a tower
   level whose activations overflow has nonfinite_px[level] > 0, an overflowing low-resolution branch nonfinite_low_px > 0, and a
   branch / level that is in range counts nothing (a coarse level's NaN is clamped before the next level reads the map);
guard band (and k = -8, where up to 19 % of a tensor is subnormal in fp16): (a), (u), (p) only, the outcome recorded.
One overflowing tower point and one overflowing low point also go through submit / wait, infer_conf, infer_lrc, a batch of 3 and
an enqueue-only call on a caller's stream.  Nothing here provokes a fault: overflow is IEEE arithmetic on valid memory.
The table (every line that starts with "range|") is profiles/activation_range.txt.
Measured there: every point passes.  FP32 bit-identical to k = 0 everywhere; in range F16X3 within 2.7e-5 px and F16 within 1.3e-3 px
(max over the map) of their k = 0 maps, nothing flagged; every overflowing point SN_ERR_RANGE in the three fp16 modes with the branch
or level named; tower k = 14 and low k = 13 (guard band) overflow in places and are flagged, k = 13 / k = 12 do not.  Against a library
whose kernels count nothing the same points fail with "SN_OK, unflagged, E 3.566e+01 >= 0.001"."""
import numpy as np
import pytest

import truth_compare as tc
from hobot_stereonet_amd import api, spec, weights

pytestmark = pytest.mark.gpu

MODES = [("fp32", api.PREC_FP32), ("f16x3", api.PREC_F16X3), ("f16", api.PREC_F16), ("auto", api.PREC_DEFAULT)]
INV_Q = np.float32(1.0 / (192.0 * float(np.float32(spec.OUT_SCALE))))
W, H, D = tc.SHAPE_S
_base = {}


def _model(tmp_path, blob):
    p = str(tmp_path / "m.snw")
    weights.save_snw(p, blob, W, H, D)
    return p


def _wire_ok(disp, raw):
    return bool(np.isfinite(disp).all() and raw.min() >= 0 and (raw == np.rint(disp * INV_Q).astype(np.int32)).all())


def _run_modes(tmp_path, blob, levels, x, x_other):
    try:
        return {m: tc.run_engine(_model(tmp_path, blob), prec, x, x_other, levels) for m, prec in MODES}
    except api.StereoNetError as e:
        if e.code == -4:              # SN_ERR_DEVICE: nothing more is started on a device that reported an error
            pytest.exit(f"device error, the session ends here: {e}", 3)
        raise


def _base_maps(tmp_path, levels, x, x_other):
    """the k = 0 run of a model, every mode, once per process"""
    if levels not in _base:
        _base[levels] = _run_modes(tmp_path, tc.range_blob(tc.RANGE_BASE[levels]), levels, x, x_other)
    return _base[levels]


def _ungauged(stages, k_low):
    """the stages under the k = 0 names: the feature maps are the one readout that carries the low gauge (x 2^k_low, exactly)"""
    return {s: a * np.float32(2.0 ** -k_low) if s.startswith("feat") else a for s, a in stages.items()}


def _flags(st):
    return list(st["nonfinite_px"]), int(st["nonfinite_low_px"])


@pytest.mark.parametrize("name", list(tc.RANGE))
def test_modes_against_the_truth_along_the_activation_range(oracle, tmp_path, name):
    levels, kt, kl, only = tc.RANGE[name]
    blob, _, prof = tc.range_point(name)
    x, x_other, r = tc.range_refs(oracle, levels)
    truth = r.truth["disp"]
    cls = tc.point_class(prof)
    record_only = cls == "guard band"
    lv_cls = {k: tc.range_class(*prof["levels"][k]) for k in range(levels)}
    low_cls = tc.range_class(*prof["low"])
    base = _base_maps(tmp_path, levels, x, x_other)
    got = base if name == tc.RANGE_BASE[levels] else _run_modes(tmp_path, blob, levels, x, x_other)
    print(f"\nrange| {name:<12} {cls:<10} tower A_max {prof['tower'][0]:.3e} sub {100 * prof['tower'][1]:5.2f} %  low A_max "
          f"{prof['low'][0]:.3e} sub {100 * prof['low'][1]:5.2f} %  (k_tower {kt:+d}{'' if only is None else f' level {only} only'}, k_low {kl:+d})")
    bad = []
    for mname, _ in MODES:
        disp, raw, st, stages, live = got[mname]
        e = tc.err(disp, truth)
        ran, (nf, nf_low) = st["precision_last"], _flags(st)
        flagged = st["returned"] == "SN_ERR_RANGE"
        moved = float(np.abs(disp - base[mname][0]).max())
        print(f"range|    {mname:<6} ran {ran:<6} E/M/S {tc.fmt(e)}  returned {st['returned']:<12} nonfinite_px {nf} low {nf_low}"
              f"  residual_px {st['residual_px']:.4g}  max |map_k - map_0| {moved:.3e}")
        fail = lambda msg: bad.append(f"{mname}: {msg}")
        # a. the wire
        if not _wire_ok(disp, raw):
            fail("output not finite, negative, or raw != rint(disp * inv_q)")
        if mname != "auto" and ran != mname:
            fail(f"forced mode ran {ran}")
        # u. the universal rule
        if flagged != (any(nf) or nf_low > 0):
            fail(f"returned {st['returned']} with nonfinite_px {nf}, nonfinite_low_px {nf_low}")
        if flagged != np.isinf(st["residual_px"]):
            fail(f"returned {st['returned']} with residual_px {st['residual_px']}")
        if not flagged:
            if mname in ("fp32", "f16x3"):
                for m in tc.class_failures(r, {"disp": disp}, tc.FP32_FACTOR if mname == "fp32" else tc.X3_FACTOR, x3=mname == "f16x3"):
                    fail(f"SN_OK, unflagged, {m}")
            elif not e[0] < tc.BUDGET:
                fail(f"SN_OK, unflagged, E {e[0]:.3e} >= {tc.BUDGET:g}")
        # p. fp32 is exact along the gauge
        if mname == "fp32":
            if flagged:
                fail("SN_PREC_FP32 flagged")
            if not (np.array_equal(disp, base["fp32"][0]) and np.array_equal(raw, base["fp32"][1])):
                fail(f"map differs from the k = 0 map (max {moved:.3e}): an fp16 step inside the fp32 path, or a head weight that underflowed")
            continue
        if cls == "in range":
            if flagged:
                fail("flagged at a point that is in range")
            # c. fp32-class (f: its coarse level maps are stages of it)
            if mname == "f16x3":
                for m in tc.class_failures(r, {"disp": disp, **_ungauged(stages, kl)}, tc.X3_FACTOR, x3=True):
                    fail(m)
            # d. / f. the fp16 tower
            if ran == "f16":
                for s, a in stages.items():
                    if not np.isfinite(a).all():
                        fail(f"{s}: not finite")
                    if s.startswith("level"):
                        k, t = int(s[5:]), r.stage_truth(s)
                        es = tc.err(a.reshape(t.shape), t)
                        if not es[0] < tc.BUDGET / 2 ** k:
                            fail(f"{s}: mean {es[0]:.3e} >= {tc.BUDGET:g} / 2^{k}")
        elif cls == "overflows":
            if not flagged:
                fail("not flagged at a point whose stored activations overflow fp16")
            if low_cls == "overflows" and nf_low == 0:
                fail("the low-resolution branch overflows and nonfinite_low_px is 0")
            if low_cls == "in range" and nf_low != 0:
                fail(f"the low-resolution branch is in range and nonfinite_low_px is {nf_low}")
            for k in range(levels):
                if lv_cls[k] == "overflows" and nf[k] == 0:
                    fail(f"the tower of level {k} overflows and nonfinite_px[{k}] is 0")
                if lv_cls[k] == "in range" and low_cls == "in range" and nf[k] != 0:
                    fail(f"the tower of level {k} is in range and nonfinite_px[{k}] is {nf[k]}")
            if mname == "auto" and (ran != "f16x3" or st["reruns"] != 1 or st["switches"] != 1):
                fail(f"the default precision ran {ran}, reruns {st['reruns']}, switches {st['switches']}: not repeated in f16x3")
    if cls == "in range":
        fp32_stages = got["fp32"][3]
        for m in tc.class_failures(r, {"disp": got["fp32"][0], **_ungauged(fp32_stages, kl)}, tc.FP32_FACTOR):
            bad.append(f"fp32: {m}")
        # b. the low-resolution branch takes no mode
        for s in tc.STAGES_SINGLE:
            if not np.array_equal(got["f16"][3][s], got["f16x3"][3][s]):
                bad.append(f"{s} of F16 and F16X3 differ: the low-resolution branch takes no mode")
        # e. the default precision
        adisp, _, ast, astages, _ = got["auto"]
        aran, ae = ast["precision_last"], tc.err(adisp, truth)
        if aran not in ("f16", "f16x3"):
            bad.append(f"auto: ran {aran}")
        elif not np.array_equal(adisp, got[aran][0]):
            bad.append(f"auto: ran {aran} but its map is not the forced {aran} map (max difference {np.abs(adisp - got[aran][0]).max():.3e})")
        else:
            bad += [f"auto: ran {aran} but its {s} is not the forced {aran} mode's" for s in tc.STAGES_SINGLE
                    if not np.array_equal(astages[s], got[aran][3][s])]
        f16_e = tc.err(got["f16"][0], truth)[0]
        if not f16_e < tc.BUDGET and aran != "f16x3":
            bad.append(f"auto: ran {aran} where forced F16 has E {f16_e:.3e} >= {tc.BUDGET:g}")
    if only is not None and cls == "overflows":
        # the same model at k = 0 has no flag anywhere: the one coarse tower is what fires
        for mname in ("f16x3", "f16", "auto"):
            if base[mname][2]["returned"] != "SN_OK" or any(base[mname][2]["nonfinite_px"]) or base[mname][2]["nonfinite_low_px"]:
                bad.append(f"{mname}: the k = 0 run of the model is flagged")
    print(f"range|    -> {'recorded only' if record_only else 'judged'}: {'; '.join(bad) if bad else 'passes'}")
    assert not bad, "\n".join(bad)


# ---- the other entry points at one overflowing tower point and one overflowing low point ----------------------------------------
@pytest.mark.parametrize("prec", [api.PREC_F16, api.PREC_DEFAULT], ids=["f16", "auto"])
@pytest.mark.parametrize("name", ["S-tower+16", "S-low+16"])
def test_every_entry_point_reports_the_overflow(tmp_path, name, prec):
    import torch
    blob, _, prof = tc.range_point(name)
    assert tc.point_class(prof) == "overflows"
    tower = tc.range_class(*prof["tower"]) == "overflows"
    x = tc.domain_input(W, H, D, tc.RANGE_INPUT)
    path = _model(tmp_path, blob)

    def named(px, low, where):
        assert (px[0] > 0) if tower else (low > 0), (where, px, low)
        if tower:
            assert low == 0, (where, low)

    def stats_flagged(eng, where):
        st = eng.refine_stats()
        named(st["nonfinite_px"], st["nonfinite_low_px"], where)
        assert np.isinf(st["residual_px"]), (where, st["residual_px"])
        return st

    with api.StereoNetHIP(path, precision=prec, max_batch=3) as eng:
        with pytest.raises(api.StereoNetRangeError) as e:
            eng.infer(x)
        assert e.value.code == api.SN_ERR_RANGE and "65504" in str(e.value)
        named(e.value.nonfinite_px, e.value.nonfinite_low_px, "infer")
        one = stats_flagged(eng, "infer")
        disp1, raw1 = e.value.outputs
        assert _wire_ok(disp1, raw1)                               # the maps were written: finite, and not to be used
        # submit / wait
        raw, disp = np.empty((H, W), np.int32), np.empty((H, W), np.float32)
        ticket = eng.submit(x, raw, disp)
        with pytest.raises(api.StereoNetRangeError) as e:
            eng.wait(ticket)
        named(e.value.nonfinite_px, e.value.nonfinite_low_px, "wait")
        assert np.array_equal(disp, disp1) and np.array_equal(raw, raw1)
        with pytest.raises(api.StereoNetError) as e2:              # the ticket was consumed
            eng.wait(ticket)
        assert e2.value.code == -7
        # the one-pass post-processing calls
        for call, where in ((lambda: eng.infer_conf(x), "infer_conf"), (lambda: eng.infer_conf(x, 0.5), "infer_conf masked"),
                            (lambda: eng.infer_lrc(x), "infer_lrc")):
            with pytest.raises(api.StereoNetRangeError) as e:
                call()
            named(e.value.nonfinite_px, e.value.nonfinite_low_px, where)
        # a batch of 3: three times the single call's counts
        with pytest.raises(api.StereoNetRangeError) as e:
            eng.infer(np.stack([x, x, x]))
        st = stats_flagged(eng, "batch of 3")
        assert st["nonfinite_px"][0] == 3 * one["nonfinite_px"][0] and st["nonfinite_low_px"] == 3 * one["nonfinite_low_px"]
        assert all(np.array_equal(m, disp1) for m in e.value.outputs[0])
        # enqueue-only on a caller's stream: SN_OK at the call, the counts once the statistic is folded in
        s1 = torch.cuda.Stream()
        dx = torch.from_numpy(x.copy()).cuda()
        t_raw = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        t_disp = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        calls = eng.refine_stats()["calls"]
        eng.infer_device(1, dx.data_ptr(), t_raw.data_ptr(), t_disp.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        st = stats_flagged(eng, "enqueue-only")
        assert st["calls"] == calls + 1
        assert st["nonfinite_px"] == one["nonfinite_px"] and st["nonfinite_low_px"] == one["nonfinite_low_px"]
        assert np.array_equal(t_disp.cpu().numpy(), disp1)
        if prec == api.PREC_DEFAULT:
            assert st["precision_selected"] == "f16x3" and st["selfcheck_epe_px"] < 0       # never calibrated on a flagged pair
