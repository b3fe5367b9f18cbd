"""The default precision (SN_PREC_AUTO) over SEQUENCES of calls on one handle, against the float64 truth.  The node that
drives the library is a stream: one handle sees thousands of different frames, in batches and through sn_submit.  Every
other test of the 1e-3 px claim judges the first call of a fresh handle; here a handle lives through a call list
(truth_compare.SEQ_CALLS) that makes it switch to SN_PREC_F16X3, re-enter SN_PREC_F16 after SN_AUTO_CALM_CALLS calm calls,
calibrate itself again and switch again, and what run_forward, fold_pending, auto_selfcheck and sn_wait feed into
sn_auto_observe is replayed through the pure state machine (truth_compare.replay).  Needs an MI355X.

The frames, their truths and the premises (calm / hard, oracle within X3_TOL) are tests/test_auto_sequences.py's.  Bounds:
truth_compare.err against BUDGET = 1e-3, bit-identity to the forced modes, 1e-9 on the integer-accumulated statistic (as
tests/test_gpu_auto.py), and one derived bound, BATCH_REL, in (d).  Forced F16 / F16X3 maps and statistics of every frame
are computed once per model (`rig`).

Head gains (truth_compare.SEQ_GAIN; the limit follows the measured self-check slope, so they were picked from {2, 4, 8} after
a run that printed limit_px, profiles/auto_sequences.txt): 2 for both models.  Measured limits: single-scale 1.0 px after a
first call on zero / tex4 / min alike (the class envelope; budget / slope would be 2.27 / 1.71 / 2.01 px), hierarchical 2.9 px
(4.18 / 3.04 / 3.01).  Under the former rule, min(4 x envelope, budget / slope), the single-scale list was live at gain 4 only and
the hierarchical handle calibrated on `zero` returned `min` from the fp16 tower at 1.026e-3 px: (b) failed, the rule changed.
Measured on the committed lists: every call of (a), (b), (e) below 4.4e-4 px (f16) / 1.3e-5 px (f16x3); trajectories live at calls
(2, 12, 13); (c) fails on the parent commit's library in all four cases (residual_px = Y's / 3); (d) worst single pair 1.026e-3 px
in a hierarchical call of 8 that stayed in f16 at a mean of 4.6e-4 px (printed, not asserted: the bound is per call)."""
import collections

import numpy as np
import pytest

import truth_compare as tc
from hobot_stereonet_amd import api, spec, weights

pytestmark = pytest.mark.gpu

MODELS = list(tc.SEQ_LEVELS)
INV_Q = np.float32(1.0 / (192.0 * float(np.float32(spec.OUT_SCALE))))
# (d): the statistic of a batch against the mean of its pairs' own.  Integer accumulation of 2^-20 fixed-point commits, one per
# workgroup, of fp32 lane sums; persistent waves span pairs, so a batch partitions the pixels differently: at most a few
# thousand commits rounded by <= 2^-21 each against a sum of several thousand -> ~1e-7 relative; x100 for the fp32 lane sums
# gives 1e-5.  Measured: at most 4.33e-9 over the six batches (profiles/auto_sequences.txt), far below that bound, which is
# therefore tightened to a little over 10 x the largest measured value.
BATCH_REL = 5e-8
W, H, D = tc.SHAPE_S


def _wire_ok(disp, raw):
    return bool(np.isfinite(disp).all() and raw.min() >= 0 and (raw == np.rint(disp * INV_Q).astype(np.int32)).all())


Forced = collections.namedtuple("Forced", "disp raw residual_px level_px E")


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """model -> (model file, {(frame, mode): Forced}): every frame once on a forced F16 and a forced F16X3 handle"""
    made = {}

    def get(model):
        if model not in made:
            path = str(tmp_path_factory.mktemp("seq") / f"{model}.snw")
            weights.save_snw(path, tc.seq_blob(model), W, H, D)
            forced = {}
            for mode, prec in (("f16", api.PREC_F16), ("f16x3", api.PREC_F16X3)):
                with api.StereoNetHIP(path, precision=prec) as eng:
                    for f in tc.SEQ_KINDS:
                        x, t, _, tres = tc.seq_point(model, f)
                        disp, raw = eng.infer(x)
                        st = eng.refine_stats()
                        assert st["precision_last"] == mode and _wire_ok(disp, raw)
                        forced[f, mode] = Forced(disp, raw, st["residual_px"], st["level_px"], tc.err(disp, t["disp"])[0])
                        print(f"PROFILE forced {model} {f:<8} {mode:<6} residual {st['residual_px']:.4f} px (truth {tres:.4f}), E {forced[f, mode].E:.3e}")
            made[model] = (path, forced)
        return made[model]
    return get


def _mode_name(eng):
    return api.PREC_NAMES[eng.precision_selected]


def _judge(model, forced, f, disp, raw, st):
    """one returned map of frame f: the wire, the budget, the forced mode's bits and statistic -> list of misses, E"""
    t = tc.seq_point(model, f)[1]["disp"]
    e = tc.err(disp, t)[0]
    bad = []
    if not _wire_ok(disp, raw):
        bad.append("output not finite, negative, or raw != rint(disp * inv_q)")
    if not e < tc.BUDGET:
        bad.append(f"E {e:.3e} >= {tc.BUDGET:g} (ran {st['precision_last']}; forced f16 {forced[f, 'f16'].E:.3e}, f16x3 {forced[f, 'f16x3'].E:.3e})")
    ran = st["precision_last"]
    if ran not in ("f16", "f16x3"):
        return bad + [f"ran {ran}"], e
    if not (np.array_equal(disp, forced[f, ran].disp) and np.array_equal(raw, forced[f, ran].raw)):
        bad.append(f"ran {ran} but the map is not the forced {ran} map (max difference {np.abs(disp - forced[f, ran].disp).max():.3e})")
    if not abs(st["residual_px"] - forced[f, ran].residual_px) < 1e-9:
        bad.append(f"residual_px {st['residual_px']!r} is not the forced {ran} handle's {forced[f, ran].residual_px!r}")
    return bad, e


def _run_calls(model, path, forced, calls, tag):
    """a fresh handle of the default precision through `calls` -> (records for replay, misses)"""
    recs, bad = [], []
    with api.StereoNetHIP(path) as eng:
        assert eng.precision == api.PREC_AUTO
        for i, f in enumerate(calls):
            start = _mode_name(eng)
            disp, raw = eng.infer(tc.seq_point(model, f)[0])
            st = eng.refine_stats()
            # what the state machine saw is the statistic of the call's first run: the forced handle's in the mode it started in
            st["observed_px"] = forced[f, start].residual_px
            msgs, e = _judge(model, forced, f, disp, raw, st)
            if st["calls"] != i + 1 or st["pairs"] != i + 1:
                msgs.append(f"calls {st['calls']} pairs {st['pairs']} after call {i}")
            print(f"PROFILE {tag} {model} call {i:2d} {f:<8} residual {st['residual_px']:.4f} limit {st['limit_px']:.4f} ran {st['precision_last']:<6} "
                  f"E {e:.3e} reruns {st['reruns']} switches {st['switches']} self-check {st['selfcheck_epe_px']:.3e} / {st['selfcheck_residual_px']:.4f}")
            bad += [f"call {i} ({f}): {m}" for m in msgs]
            recs.append(st)
    return recs, bad


@pytest.mark.parametrize("model", MODELS)
def test_a_sequence_of_synchronous_calls(rig, model):
    """(a) calm x2, hard, hard, calm x9, hard, calm, noise, hard on one handle: every call is valid on the wire, below 1e-3 px,
    bit-identical to the forced mode precision_last names and carries that mode's statistic; the trajectory replays clean
    through sn_auto_* and is live (a switch with a repeat, a re-entry, a second switch)."""
    path, forced = rig(model)
    recs, bad = _run_calls(model, path, forced, tc.SEQ_CALLS, "sequence")
    bad += [f"replay, call {i}: {m}" for i, m in tc.replay(recs, tc.SEQ_LEVELS[model])]
    live = tc.trajectory_is_live(recs)
    print(f"PROFILE sequence {model} live (switch with repeat, re-entry, second switch) at calls {live}")
    assert not bad, "\n".join(bad)
    assert None not in live, live


@pytest.mark.parametrize("model", MODELS)
def test_the_order_of_the_first_frame(rig, model):
    """(b) the self-check measures ONE pair, the first the handle sees in F16, and the limit follows it: the same six frames
    started at the calmest frame, at a texture and at a hard frame.  Every call of every rotation below 1e-3 px, and no rotation
    returns the F16 map of a frame on which forced F16 is at or over the budget."""
    path, forced = rig(model)
    bad = []
    for first in tc.SEQ_ROTATIONS:
        k = tc.SEQ_ROTATED.index(first)
        calls = tc.SEQ_ROTATED[k:] + tc.SEQ_ROTATED[:k]
        recs, msgs = _run_calls(model, path, forced, calls, f"rotation-{first}")
        bad += [f"first {first}: {m}" for m in msgs]
        bad += [f"first {first}: replay, call {i}: {m}" for i, m in tc.replay(recs, tc.SEQ_LEVELS[model])]
        print(f"PROFILE rotation {model} first {first:<5} self-check EPE {recs[0]['selfcheck_epe_px']:.3e} px at residual "
              f"{recs[0]['selfcheck_residual_px']:.4f} px -> limit {recs[0]['limit_px']:.4f} px (envelope {recs[0]['envelope_px']:.2f})")
        for f, r in zip(calls, recs):
            if not forced[f, "f16"].E < tc.BUDGET and r["precision_last"] != "f16x3":
                bad.append(f"first {first}: {f} returned in {r['precision_last']} where forced F16 has E {forced[f, 'f16'].E:.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ("f16", "auto"))
@pytest.mark.parametrize("x_name,y_name", (("tex4", "min"), ("min", "tex4")))
def test_a_pending_statistic_is_not_read_as_the_next_call_s(rig, kind, x_name, y_name):
    """(c) an enqueue-only call of 3 pairs of frame X on a caller stream that is still busy, then at once a host-mode call of
    frame Y on the same stream (blocking and stream-ordered, so legal), then sn_get_refine_stats: two calls, four pairs, the
    statistic of Y alone, and a running mean and decisions that saw X's call and then Y's, each once.
    kind "f16": a forced handle — exactly these two calls.  kind "auto": the first enqueue-only call of a handle of the default
    precision blocks for its self-check and leaves nothing pending, so the handle gets one calm synchronous call (`zero`)
    first; the counts are then one call and one pair higher and the replay has three observations."""
    import ctypes as C
    import torch
    model = "single"
    path, forced = rig(model)
    x, y = tc.seq_point(model, x_name)[0], tc.seq_point(model, y_name)[0]
    x3 = np.ascontiguousarray(np.stack([x] * 3))
    warm = 1 if kind == "auto" else 0
    stream = torch.cuda.Stream()
    dx = torch.from_numpy(x3).cuda()
    out = torch.empty((3, H, W), dtype=torch.int32, device="cuda")
    busy = torch.randn(6144, 6144, device="cuda")
    torch.cuda.synchronize()
    with api.StereoNetHIP(path, max_batch=3, precision=api.PREC_F16 if kind == "f16" else api.PREC_DEFAULT) as eng:
        recs = []
        if warm:
            eng.infer(tc.seq_point(model, "zero")[0])
            st = eng.refine_stats()
            st["observed_px"] = forced["zero", "f16"].residual_px
            assert st["precision_last"] == "f16" and st["precision_selected"] == "f16", st
            recs.append(st)
        x_mode = _mode_name(eng)
        with torch.cuda.stream(stream):
            for _ in range(4):
                busy = busy @ busy * 1e-4                 # the caller's own work: the handle's event cannot be ready yet
        eng.infer_device(3, dx.data_ptr(), out.data_ptr(), 0, stream.cuda_stream)
        disp, raw = np.empty((H, W), np.float32), np.empty((H, W), np.int32)
        rc = eng._lib.sn_infer_batch(eng._h, 1, y.ctypes.data, raw.ctypes.data, disp.ctypes.data, api.SN_MEM_HOST,
                                     C.c_void_p(stream.cuda_stream))
        assert rc == 0, eng._lib.sn_last_error(eng._h)
        st = eng.refine_stats()
        stream.synchronize()
    # the statistic of the same 3-pair call when nobody disturbs it
    with api.StereoNetHIP(path, max_batch=3, precision=api.PREC_F16 if x_mode == "f16" else api.PREC_F16X3) as eng:
        eng.infer(x3)
        x_res = eng.refine_stats()["residual_px"]
    y_start = "f16"
    if kind == "auto":
        # the two observations in order, through the pure state machine: X's call (never repeated: it was only enqueued), Y's
        s, lib = api.SnAutoState(), api.load_library()
        lib.sn_auto_init(C.byref(s), 1)
        s.epe_per_px = recs[0]["selfcheck_epe_px"] / recs[0]["selfcheck_residual_px"]
        lib.sn_auto_observe(C.byref(s), recs[0]["observed_px"])
        y_start = api.PREC_NAMES[lib.sn_auto_observe(C.byref(s), x_res)]
        y_res = forced[y_name, y_start].residual_px
        after = lib.sn_auto_observe(C.byref(s), y_res)
        y_last = "f16x3" if (y_start == "f16" and after == api.PREC_F16X3) else y_start
        want = {"switches": s.switches, "precision_selected": api.PREC_NAMES[s.mode], "running_px": s.running_px,
                "reruns": int(y_start == "f16" and y_last == "f16x3"), "precision_last": y_last}
    else:
        y_res = forced[y_name, "f16"].residual_px
        want = {"switches": 0, "precision_selected": "f16", "running_px": 0.75 * x_res + 0.25 * y_res, "reruns": 0, "precision_last": "f16"}
    print(f"PROFILE pending {kind} X {x_name} (3 pairs, {x_mode}, residual {x_res:.6f}) then Y {y_name}: residual_px {st['residual_px']:.6f} "
          f"(Y alone in {want['precision_last']}: {forced[y_name, want['precision_last']].residual_px:.6f}), running_px {st['running_px']:.6f} "
          f"(want {want['running_px']:.6f}), switches {st['switches']} (want {want['switches']}), selected {st['precision_selected']}, ran {st['precision_last']}")
    assert st["calls"] == warm + 2 and st["pairs"] == warm + 4, st
    y_forced = forced[y_name, want["precision_last"]]
    assert abs(st["residual_px"] - y_forced.residual_px) < 1e-9, (st["residual_px"], y_forced.residual_px, y_forced.residual_px * 1 / 3)
    assert all(abs(a - b) < 1e-9 for a, b in zip(st["level_px"], y_forced.level_px)), (st["level_px"], y_forced.level_px)
    assert abs(st["running_px"] - want["running_px"]) < 1e-9, (st["running_px"], want["running_px"])
    for k in ("switches", "precision_selected", "reruns", "precision_last"):
        assert st[k] == want[k], (k, st[k], want[k], st)
    assert np.array_equal(raw, y_forced.raw) and np.array_equal(disp, y_forced.disp)
    xo = out.cpu().numpy()
    assert all(np.array_equal(xo[i], forced[x_name, x_mode].raw) for i in range(3))


CALM7 = ("zero", "tex4", "tex5", "tex6", "zero", "tex4", "tex5")
BATCHES = {"7 calm + 1 hard": CALM7 + ("min",), "8 calm + 1 hard in the second chunk": CALM7 + ("tex6", "max"),
           "all hard": ("max", "step", "min") * 3}


@pytest.mark.parametrize("model", MODELS)
def test_mixed_batches(rig, model):
    """(d) max_batch = 9, so that a call crosses the 8-pair refinement chunk.  The rule and the bound are per CALL, on the mean
    over its pairs (include/stereonet_hip.h): the call's residual_px is the mean of its pairs' own within BATCH_REL, every
    pair's map is bit-identical to the forced mode precision_last names, and the mean E of the call's pairs is below 1e-3 px.
    The worst single pair is printed (profiles/auto_sequences.txt), not asserted: a per-pair statistic is a follow-up."""
    path, forced = rig(model)
    bad = []
    for name, frames in BATCHES.items():
        xs = np.stack([tc.seq_point(model, f)[0] for f in frames])
        with api.StereoNetHIP(path, max_batch=9) as eng:
            disp, raw = eng.infer(xs)
            st = eng.refine_stats()
        ran = st["precision_last"]
        es = [tc.err(disp[i], tc.seq_point(model, f)[1]["disp"])[0] for i, f in enumerate(frames)]
        singles = float(np.mean([forced[f, ran].residual_px for f in frames]))
        rel = abs(st["residual_px"] - singles) / singles
        worst = int(np.argmax(es))
        print(f"PROFILE batch {model} '{name}': ran {ran}, residual_px {st['residual_px']:.6f} vs mean of the pairs' own {singles:.6f} (relative "
              f"difference {rel:.2e}), limit {st['limit_px']:.4f}, reruns {st['reruns']}, mean E {np.mean(es):.3e}, worst pair {worst} ({frames[worst]}) "
              f"E {es[worst]:.3e}" + (" — OVER 1e-3 in a call that stayed in f16" if ran == "f16" and not es[worst] < tc.BUDGET else ""))
        if st["calls"] != 1 or st["pairs"] != len(frames):
            bad.append(f"{name}: calls {st['calls']} pairs {st['pairs']}")
        if not rel < BATCH_REL:
            bad.append(f"{name}: residual_px {st['residual_px']!r} vs the mean of the single-pair residuals {singles!r}: relative {rel:.3e}")
        for i, f in enumerate(frames):
            if not _wire_ok(disp[i], raw[i]):
                bad.append(f"{name} pair {i} ({f}): output not finite, negative, or raw != rint(disp * inv_q)")
            if not (np.array_equal(disp[i], forced[f, ran].disp) and np.array_equal(raw[i], forced[f, ran].raw)):
                bad.append(f"{name} pair {i} ({f}): ran {ran} but the map is not the forced {ran} map")
        if not np.mean(es) < tc.BUDGET:
            bad.append(f"{name}: mean E {np.mean(es):.3e} >= {tc.BUDGET:g} (ran {ran})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("model", MODELS)
def test_the_sequence_through_submit_and_wait(rig, model):
    """(e) the call list of (a) through sn_submit / sn_wait with three slots and three tickets in flight: every map below
    1e-3 px and bit-identical to the forced F16 or F16X3 map of its frame; every ticket counted; a ticket submitted in F16X3 comes
    back in F16X3, and reruns counts exactly the tickets that were submitted in F16 and came back in F16X3.  Every submit has a
    finite timeout: a slot that a wait did not hand back fails the test (SN_ERR_BUSY) instead of hanging it."""
    path, forced = rig(model)
    bad, flight, done = [], collections.deque(), []

    def collect(eng):
        i, f, t, raw, disp, start = flight.popleft()
        eng.wait(t)
        done.append((i, f, raw, disp, start))

    with api.StereoNetHIP(path, task_num=3) as eng:
        for i, f in enumerate(tc.SEQ_CALLS):
            if len(flight) == 3:
                collect(eng)
            raw, disp = np.empty((H, W), np.int32), np.empty((H, W), np.float32)
            start = _mode_name(eng)
            flight.append((i, f, eng.submit(tc.seq_point(model, f)[0], raw, disp, timeout_ms=20000), raw, disp, start))
        while flight:
            collect(eng)
        st = eng.refine_stats()
    repeated = 0
    for i, f, raw, disp, start in done:
        e = tc.err(disp, tc.seq_point(model, f)[1]["disp"])[0]
        same = [m for m in ("f16", "f16x3") if np.array_equal(raw, forced[f, m].raw) and np.array_equal(disp, forced[f, m].disp)]
        print(f"PROFILE async {model} ticket {i:2d} {f:<8} submitted in {start:<6} returned {'/'.join(same) or 'NEITHER'} E {e:.3e}")
        if not _wire_ok(disp, raw):
            bad.append(f"ticket {i} ({f}): output not finite, negative, or raw != rint(disp * inv_q)")
        if not e < tc.BUDGET:
            bad.append(f"ticket {i} ({f}): E {e:.3e} >= {tc.BUDGET:g}")
        if not same:
            bad.append(f"ticket {i} ({f}): neither the forced F16 nor the forced F16X3 map")
        elif start == "f16x3" and "f16x3" not in same:
            bad.append(f"ticket {i} ({f}): submitted in f16x3, returned the f16 map")
        elif start == "f16" and same == ["f16x3"]:
            repeated += 1
    print(f"PROFILE async {model}: calls {st['calls']} reruns {st['reruns']} (tickets submitted in f16 and returned in f16x3: {repeated}) "
          f"switches {st['switches']} selected {st['precision_selected']}")
    assert not bad, "\n".join(bad)
    assert st["calls"] == len(tc.SEQ_CALLS) and st["pairs"] == len(tc.SEQ_CALLS)
    assert st["reruns"] == repeated >= 1
    assert st["switches"] >= 2                          # it left F16 and came back


@pytest.mark.parametrize("model", MODELS)
def test_the_other_entry_points_that_run_forwards(rig, model):
    """(f) sn_infer_conf and sn_infer_lrc on a handle that sits in F16 (one calm call before), for a hard and a calm frame: the
    rule sends the hard one to F16X3 and keeps the calm one.  infer_conf: map, confidence, mask and kept count are the forced
    handle's in the mode precision_last names.  infer_lrc: two calls counted, and its left map is infer's map of that frame in
    that mode wherever the check kept the pixel (rejected pixels are 0)."""
    path, forced = rig(model)
    for f in ("min", "tex5"):
        x = tc.seq_point(model, f)[0]
        t = tc.seq_point(model, f)[1]["disp"]
        for entry in ("conf", "lrc"):
            with api.StereoNetHIP(path) as eng:
                eng.infer(tc.seq_point(model, "zero")[0])
                st0 = eng.refine_stats()
                assert st0["precision_selected"] == "f16" and st0["calls"] == 1
                want = "f16x3" if forced[f, "f16"].residual_px > st0["limit_px"] else "f16"
                if entry == "conf":
                    got = eng.infer_conf(x, min_conf=0.5)
                    st = eng.refine_stats()
                    assert st["calls"] == 2 and st["precision_last"] == want, (f, want, st)
                    assert st["reruns"] == (1 if want == "f16x3" else 0)
                else:
                    disp, raw, mask, kept = eng.infer_lrc(x, tau_px=1000.0)       # keep whatever has a partner
                    st = eng.refine_stats()
                    assert st["calls"] == 3 and st["pairs"] == 3, st
            if entry == "conf":
                with api.StereoNetHIP(path, precision=api.PREC_F16 if want == "f16" else api.PREC_F16X3) as ref:
                    exp = ref.infer_conf(x, min_conf=0.5)
                for name, a, b in zip(("disp", "raw", "conf", "mask", "kept"), got, exp):
                    assert np.array_equal(a, b), (f, want, name)
                print(f"PROFILE entry {model} infer_conf {f}: ran {want}, kept {int(got[4][0])} px, all five outputs are the forced {want} handle's")
            else:
                k = mask == api.SN_LRC_KEPT
                assert kept[0] == k.sum() > 0 and not raw[~k].any()
                assert np.array_equal(raw[k], forced[f, want].raw[k]) and np.array_equal(disp[k], forced[f, want].disp[k]), (f, want)
                other = "f16" if want == "f16x3" else "f16x3"
                assert not np.array_equal(raw[k], forced[f, other].raw[k])           # the comparison can tell the two modes apart
                e = tc.err(np.where(k, disp, 0), np.where(k, t, 0))[0]
                print(f"PROFILE entry {model} infer_lrc {f}: left map is the forced {want} map on the {int(kept[0])} kept px (E over them {e:.3e})")
                assert e < tc.BUDGET
