"""The temporal filter's numpy twin (hobot_stereonet_amd/temporal.py) against a per-pixel Python loop written from the header
text of sn_temporal_push (tests/golden/plain_refs.py), hand-computed pixel histories, the mask values the test clip must produce (the condition that keeps
the GPU comparison from passing on an idle filter), interleaved streams, what the filter buys on the clip's static part, and
the binding against the header.  No GPU."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import api, dispfilter, temporal
from hobot_stereonet_amd.temporal import BLENDED, HELD, INVALID_IN, JUMP, MOVED
from plain_refs import temporal_loop as _loop

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31
S = float(temporal.wire_scale())
# (alpha, q, persist, luma_delta) with q = delta_px in raw units, and the mask values the clip must produce for each
SETTINGS = {(64, 1000, 2, 24): {0, 1, 2, 5, 8, 9, 16}, (256, 0, 1, 0): {0, 1, 5, 16},
            (128, 400, 0, 24): {0, 1, 2, 8, 9, 16}, (64, 1000, 8, 0): {0, 1, 2, 5, 16}}


def _corner_clip(seed):
    rng = np.random.default_rng(seed)
    vals = np.array([IMIN, -7, -1, 0, 0, 0, 1, 1, 2, IMAX, IMAX - 1, 1000, 1000, 1001, 1900, 2100, 2100], np.int64)
    raw = vals[rng.integers(0, len(vals), (12, 16, 24))].astype(np.int32)
    raw[:, 0, :4] = np.array([[IMAX, 1, IMIN, 0]] * 6 + [[1, IMAX, IMAX, IMAX]] * 6)      # IMAX beside 1, frame after frame
    lumas = np.array([0, 10, 11, 40, 200, 255, 255], np.uint8)
    luma = lumas[rng.integers(0, len(lumas), raw.shape)]
    return raw, luma


def test_twin_equals_the_per_pixel_loop_over_the_parameter_grid():
    raw, luma = _corner_clip(3)
    seen = set()
    for delta_px, q in ((0.0, 0), (temporal.delta_for(1000), 1000), (3.0e38, 2 ** 32)):
        assert dispfilter.diff_units(delta_px) == q                             # the cap is hit: 2^32
        for alpha, persist, luma_delta in itertools.product((1, 64, 255, 256), (0, 1, 2, 8), (0, 1, 24, 255)):
            if q == 1000 and (alpha, persist) not in ((64, 2), (255, 8)):      # the middle threshold: a sample of the grid
                continue
            out, mask, counts = temporal.reference(raw, luma, (alpha, delta_px, persist, luma_delta))
            w_out, w_mask = _loop(raw, luma, alpha, q, persist, luma_delta)
            tag = (alpha, q, persist, luma_delta)
            assert np.array_equal(out, w_out) and np.array_equal(mask, w_mask), tag
            assert out.dtype == np.int32 and mask.dtype == np.uint8 and counts.dtype == np.uint32 and counts.shape == (12, 4)
            assert np.array_equal(counts, temporal.counts_of(w_out, w_mask)), tag
            assert out[mask & BLENDED != 0].min(initial=1) >= 1                 # a blend is never 0
            assert np.array_equal(out > 0, np.isin(mask, (0, 2, 5, 8, 16))), tag
            seen |= set(np.unique(mask).tolist())
    assert seen == set(temporal.MASK_VALUES)
    # the 64-bit blend of the largest values: INT32_MAX with 1, every alpha
    for alpha in (1, 64, 255, 256):
        st = temporal.TemporalState(1, 2)
        st.push(np.array([[IMAX, 1]], np.int32), None, alpha, 2 ** 32, 0, 0)
        o, m = st.push(np.array([[1, IMAX]], np.int32), None, alpha, 2 ** 32, 0, 0)
        want = [(alpha * 1 + (256 - alpha) * IMAX + 128) >> 8, (alpha * IMAX + (256 - alpha) * 1 + 128) >> 8]
        assert o[0].tolist() == want and all(1 <= x <= IMAX for x in want)
        assert m[0].tolist() == [0 if x == y else 2 for x, y in zip(want, (1, IMAX))]


def _history(values, lumas, params):
    raw = np.array(values, np.int32).reshape(-1, 1, 1)
    luma = None if lumas is None else np.array(lumas, np.uint8).reshape(-1, 1, 1)
    out, mask, _ = temporal.reference(raw, luma, params)
    return out.ravel().tolist(), mask.ravel().tolist()


def test_hand_computed_pixel_histories():
    # a hold ends after Hs empties: one measurement, then nothing.  Frames 1..8 see the measurement's bit in Hs and hold; frame 8
    # shifts it out (Hs' == 0 clears P), so frame 9 has nothing to hold: a held value is never older than eight frames
    assert _history([500] + [0] * 10, None, (256, 0.0, 1, 0)) == ([500] * 9 + [0, 0], [0] + [5] * 8 + [1, 1])
    # persist = 2 needs two valid inputs among the last eight: one is not enough, two are, and the hold lasts until the
    # SECOND-last of them leaves the history (frames 2..8; at frame 9 only one bit is left)
    assert _history([500, 0], None, (256, 0.0, 2, 0)) == ([500, 0], [0, 1])
    assert _history([500, 500] + [0] * 9, None, (256, 0.0, 2, 0)) == ([500, 500] + [500] * 7 + [0, 0], [0, 0] + [5] * 7 + [1, 1])
    # persist = 0 never fills
    assert _history([500, 0, 0], None, (256, 0.0, 0, 0)) == ([500, 0, 0], [0, 1, 1])
    # a blend that rounds at .5: (128*3 + 128*2 + 128) >> 8 = 3 (2.5 goes up; out == r, so no BLENDED bit), and
    # (64*1002 + 192*1000 + 128) >> 8 = 1001 (1000.5 goes up); then (64*1000 + 192*1001 + 128) >> 8 = 1001 (1000.75)
    big = temporal.delta_for(5000)
    assert _history([2, 3], None, (128, big, 0, 0)) == ([2, 3], [0, 0])
    assert _history([1000, 1002, 1000], None, (64, big, 0, 0)) == ([1000, 1001, 1001], [0, 2, 2])
    # |r - P| against q: 1000 apart blends at q = 1000, 1001 apart is a jump
    q1000 = temporal.delta_for(1000)
    assert _history([5000, 6000], None, (128, q1000, 0, 0)) == ([5000, 5500], [0, 2])
    assert _history([5000, 6001], None, (128, q1000, 0, 0)) == ([5000, 6001], [0, 16])
    # a first frame never counts as moved, whatever its luma (there is no previous luma), valid or not ...
    assert _history([700, 700], [255, 255], (128, big, 1, 1)) == ([700, 700], [0, 0])
    assert _history([0, 700], [255, 255], (128, big, 1, 1)) == ([0, 700], [1, 0])
    # ... and the second frame does: a valid pixel is taken as it is (MOVED), an invalid one drops its past (INVALID_IN | MOVED)
    # instead of holding it, so the frame after has nothing to hold either
    assert _history([700, 900, 900], [10, 12, 12], (128, big, 1, 1)) == ([700, 900, 900], [0, 8, 0])
    assert _history([700, 0, 0], [10, 12, 12], (128, big, 1, 1)) == ([700, 0, 0], [0, 9, 1])
    assert _history([700, 0, 0], [10, 11, 11], (128, big, 1, 1)) == ([700, 700, 700], [0, 5, 5])      # |dy| == luma_delta: not moved
    # a negative input is no measurement: out 0, and it counts as invalid in the history
    assert _history([-5, 40, -5], None, (256, 0.0, 1, 0)) == ([0, 40, 40], [1, 0, 5])


@pytest.mark.parametrize("w,h", [(96, 64), (1242, 375)])
def test_noisy_sequence_produces_every_mask_value_of_every_setting(w, h):
    raw, luma, truth = temporal.noisy_sequence(w, h, 12, w + h)
    assert raw.shape == luma.shape == truth.shape == (12, h, w) and raw.dtype == np.int32 and luma.dtype == np.uint8
    assert (raw < 0).any() and (raw == 0).any() and not temporal.static_part(truth).all() and temporal.static_part(truth).any()
    for (alpha, q, persist, luma_delta), values in SETTINGS.items():
        _, mask, _ = temporal.reference(raw, luma, (alpha, temporal.delta_for(q), persist, luma_delta))
        got = dict(zip(*[a.tolist() for a in np.unique(mask, return_counts=True)]))
        print(f"{w}x{h} {(alpha, q, persist, luma_delta)}: {got}")
        assert set(got) == values


def test_interleaved_streams_equal_per_stream_clips():
    raw, luma, _ = temporal.noisy_sequence(48, 32, 12, 5)
    params = (64, temporal.delta_for(1000), 2, 24)
    ids = [0, 2, 1, 1, 0, 2, 2, 2, 0, 1, 0, 1]
    out, mask, counts = temporal.reference(raw, luma, params, ids)
    for s in range(3):
        sel = [k for k in range(12) if ids[k] == s]
        o, m, c = temporal.reference(raw[sel], luma[sel], params)
        assert np.array_equal(out[sel], o) and np.array_equal(mask[sel], m) and np.array_equal(counts[sel], c)
    # a call equals single pushes, and `states` carries a stream across calls
    states = {}
    a = temporal.reference(raw[:5], luma[:5], params, ids[:5], states)
    b = temporal.reference(raw[5:], luma[5:], params, ids[5:], states)
    assert np.array_equal(np.concatenate([a[0], b[0]]), out) and np.array_equal(np.concatenate([a[1], b[1]]), mask)
    for bad in ((0, 0.5, 2, 24), (257, 0.5, 2, 24), (64, -1.0, 2, 24), (64, float("nan"), 2, 24), (64, 0.5, 9, 24), (64, 0.5, 2, 256)):
        with pytest.raises(ValueError):
            temporal.reference(raw, luma, bad)
    with pytest.raises(ValueError):
        temporal.reference(raw, None, params)                                   # luma_delta > 0 needs the luma
    assert temporal.reference(raw, None, (64, 0.5, 2, 0))[0].shape == raw.shape


@pytest.mark.parametrize("w,h", [(96, 64), (1242, 375)])
def test_filter_lowers_error_and_flicker_on_the_static_part(w, h):
    raw, luma, truth = temporal.noisy_sequence(w, h, 12, w + h)
    out, mask, _ = temporal.reference(raw, luma, (64, temporal.delta_for(1000), 2, 24))
    still = temporal.static_part(truth)[None]
    r = np.maximum(raw, 0)
    err_in = float(np.abs(r - truth)[(r > 0) & still].mean())
    err_out = float(np.abs(out - truth)[(out > 0) & still].mean())
    fl_in, fl_out = temporal.flicker(np.where(still, r, 0)), temporal.flicker(np.where(still, out, 0))
    print(f"{w}x{h} static part: error {err_in * S:.4f} -> {err_out * S:.4f} px (ratio {err_out / err_in:.3f}), "
          f"flicker {fl_in * S:.4f} -> {fl_out * S:.4f} px (ratio {fl_out / fl_in:.3f}), "
          f"density {float((r > 0).mean()):.3f} -> {float((out > 0).mean()):.3f}")
    assert err_out < err_in and fl_out < fl_in
    # pixels > 0 in both frames only: |1 - 4| between frames 0 and 1, |3 - 1| and |9 - 5| between frames 1 and 2
    assert temporal.flicker(np.array([[[4, 0, 7]], [[1, 5, 0]], [[3, 9, 9]]])) == 3.0
    assert np.isnan(temporal.flicker(np.zeros((3, 2, 2), np.int32)))


def test_expected_disp_rewrites_exactly_the_changed_pixels():
    raw = np.array([[[-3, 0, 500, 700]]], np.int32)
    out = np.array([[[0, 650, 500, 690]]], np.int32)
    d0 = np.array([[[1.0, 2.0, 3.0, 4.0]]], np.float32)
    got = temporal.expected_disp(d0, raw, out)
    s = temporal.wire_scale()
    assert got.ravel().tolist() == [1.0, float(np.float32(650) * s), 3.0, float(np.float32(690) * s)]


def test_temporal_binding_agrees_with_the_header():
    enums = {k: int(v) for k, v in re.findall(r"\b(SN_TMP_[A-Z0-9_]+)\s*=\s*(\d+)", HEADER)}
    assert enums == {"SN_TMP_INVALID_IN": 1, "SN_TMP_BLENDED": 2, "SN_TMP_HELD": 4, "SN_TMP_MOVED": 8, "SN_TMP_JUMP": 16}
    for name, value in enums.items():
        assert getattr(api, name) == value, name
    assert (INVALID_IN, BLENDED, HELD, MOVED, JUMP) == (1, 2, 4, 8, 16)
    assert "PLANE OF ITS OWN" in HEADER                                         # the chain's OR-able mask has no bit left
    body = re.search(r"typedef struct sn_temporal_params \{(.*?)\} sn_temporal_params;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    ctype = {"float": C.c_float, "int": C.c_int}
    assert [(name, ctype[t]) for t, name in decls] == list(api.SnTemporalParams._fields_)
    assert C.sizeof(api.SnTemporalParams) == 16 and temporal.Params._fields == tuple(n for n, _ in api.SnTemporalParams._fields_)
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # 4: SN_ERR_RANGE and the range counts of sn_refine_stats; these structs are as in 3
    assert "typedef struct sn_temporal sn_temporal;" in HEADER
    lib = api.load_library()
    protos = {
        "sn_temporal_create": (["sn_handle *h", "int streams", "const sn_temporal_params *p", "sn_temporal **out"], C.c_int),
        "sn_temporal_reset": (["sn_temporal *t", "int stream"], C.c_int),
        "sn_temporal_destroy": (["sn_temporal *t"], None),
        "sn_temporal_push": (["sn_temporal *t", "int n", "const int *stream_of", "const int32_t *raw", "const void *guide",
                              "int guide_kind", "int guide_pitch", "int32_t *out_raw", "float *disp_inout", "uint8_t *mask",
                              "uint32_t *counts", "int mem", "void *stream"], C.c_int)}
    for name, (params, restype) in protos.items():
        ret = "void" if restype is None else "int"
        proto = re.search(r"\b%s\s+%s\((.*?)\);" % (ret, name), HEADER, re.S).group(1)
        assert [" ".join(t.split()) for t in proto.split(",")] == params, name
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == len(params), name
        for at, prm in zip(fn.argtypes, params):
            if prm.startswith("int "):
                assert at is C.c_int, (name, prm)
            elif "sn_temporal_params" in prm:
                assert at is C.POINTER(api.SnTemporalParams)
            elif prm == "sn_temporal **out":
                assert at is C.POINTER(C.c_void_p)
            else:
                assert at is C.c_void_p, (name, prm)
    assert all(callable(getattr(api.TemporalFilter, f)) for f in ("push", "push_device", "reset", "close"))
    assert callable(api.StereoNetHIP.temporal_filter)


def test_compat_builds_the_temporal_harness():
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    assert os.path.exists(os.path.join(COMPAT, "build", "temporal_harness"))
    src = open(os.path.join(COMPAT, "src", "stereonet_node.cpp")).read()
    assert "STEREONET_TEMPORAL" in src and "sn_temporal_push" in src


@pytest.mark.parametrize("value", ["0,1", "64", "64,x", "64,-1", "64,nan", "64,1,9", "64,1,2,256", "64,1,2,3,4", "257,1", "6.5,1"])
def test_filelist_rejects_bad_temporal_arguments_before_any_work(value, capsys):
    from hobot_stereonet_amd import filelist
    with pytest.raises(SystemExit):
        filelist.main(["--model", "none.snw", "--left", "none.list", "--right", "none.list", "--temporal", value])
    assert "--temporal takes ALPHA" in capsys.readouterr().err
