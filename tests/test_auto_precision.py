"""SN_PREC_AUTO's decision (include/stereonet_hip.h: sn_auto_*) as pure functions — no GPU.  The reference loads an opaque
model_file (stereonet_infer/src/stereonet_node.cpp:131-136); the default precision of this library therefore watches the
refinement statistic and leaves the fp16 tower when it says the tower's error would exceed north_star's 1e-3 px.  Here: the
state machine (switch up at once, switch down only after SN_AUTO_CALM_CALLS calm calls), the effect of the self-check's
measured slope on the limit, and the struct layouts the Python binding mirrors."""
import ctypes as C
import re
import os

import pytest

from hobot_stereonet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()


def _define(name):
    m = re.search(rf"#define\s+{name}\s+([0-9.eE+-]+)", HEADER)
    assert m, name
    return float(m.group(1))


BUDGET, REENTRY, CALM = _define("SN_AUTO_BUDGET_PX"), _define("SN_AUTO_REENTRY"), int(_define("SN_AUTO_CALM_CALLS"))


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


def _state(lib, levels=1):
    s = api.SnAutoState()
    assert lib.sn_auto_init(C.byref(s), levels) == 0
    return s


def test_abi_version_and_default_precision_are_the_header_s(lib):
    assert lib.sn_abi_version() == api.ABI_VERSION == int(_define("SN_ABI_VERSION"))
    assert re.search(r"SN_PREC_AUTO\s*=\s*4", HEADER) and api.PREC_AUTO == 4
    assert "selects SN_PREC_AUTO" in HEADER


def test_init(lib):
    for levels in (1, 4):
        s = _state(lib, levels)
        assert s.mode == api.PREC_F16 and s.calm == 0 and s.switches == 0 and s.epe_per_px == 0.0 and s.running_px < 0
        assert s.envelope_px == lib.sn_auto_envelope_px(levels) > 0
        assert lib.sn_auto_limit_px(C.byref(s)) == s.envelope_px
    assert lib.sn_auto_init(None, 1) < 0 and lib.sn_auto_observe(None, 1.0) < 0


def test_inside_the_envelope_nothing_happens(lib):
    s = _state(lib)
    for _ in range(100):
        assert lib.sn_auto_observe(C.byref(s), 0.7 * s.envelope_px) == api.PREC_F16
    assert s.switches == 0
    assert abs(s.running_px - 0.7 * s.envelope_px) < 1e-12


def test_one_call_outside_switches_at_once_and_the_way_back_needs_calm_calls(lib):
    s = _state(lib)
    env = s.envelope_px
    assert lib.sn_auto_observe(C.byref(s), 1.01 * env) == api.PREC_F16X3          # the caller repeats that call
    assert s.switches == 1
    # inside the envelope but outside the re-entry band: stays
    for _ in range(3 * CALM):
        assert lib.sn_auto_observe(C.byref(s), 0.9 * env) == api.PREC_F16X3
    # calm calls are counted consecutively: one call outside the band resets the count
    for _ in range(CALM - 1):
        assert lib.sn_auto_observe(C.byref(s), 0.5 * REENTRY * env) == api.PREC_F16X3
    assert lib.sn_auto_observe(C.byref(s), 0.95 * env) == api.PREC_F16X3
    for i in range(CALM):
        m = lib.sn_auto_observe(C.byref(s), 0.5 * REENTRY * env)
        assert m == (api.PREC_F16 if i == CALM - 1 else api.PREC_F16X3)
    assert s.switches == 2 and s.calm == 0


def test_the_self_check_tightens_the_limit(lib):
    s = _state(lib)
    env = s.envelope_px
    # a model whose fp16 tower loses 2e-3 px per pixel of residual: the limit is the budget over that slope
    s.epe_per_px = 2e-3
    lim = lib.sn_auto_limit_px(C.byref(s))
    assert abs(lim - BUDGET / 2e-3) < 1e-12 and lim < env      # (every class envelope is above 0.425 px)
    assert lib.sn_auto_observe(C.byref(s), 0.9 * lim) == api.PREC_F16
    assert lib.sn_auto_observe(C.byref(s), 1.1 * lim) == api.PREC_F16X3
    # a benign self-check pair widens nothing: the slope of one pair says little about the next frame's
    # (tests/test_gpu_auto_sequences.py), so the limit never exceeds the class envelope
    t = _state(lib)
    for slope in (BUDGET / (2.0 * env), BUDGET / (1.0001 * env), 1e-6, 1e-300):
        t.epe_per_px = slope
        assert lib.sn_auto_limit_px(C.byref(t)) == env
        assert lib.sn_auto_observe(C.byref(t), 0.99 * env) == api.PREC_F16
    assert lib.sn_auto_observe(C.byref(t), 1.01 * env) == api.PREC_F16X3
    t.epe_per_px = BUDGET / (0.9999 * env)                  # continuous where the two meet
    assert abs(lib.sn_auto_limit_px(C.byref(t)) - 0.9999 * env) < 1e-12
    assert "SN_AUTO_ENVELOPE_CAP" not in HEADER


def test_garbage_statistics_are_not_trusted(lib):
    for bad in (float("nan"), -1.0, float("inf")):
        s = _state(lib)
        assert lib.sn_auto_observe(C.byref(s), bad) == api.PREC_F16X3


def test_struct_layouts_match_the_header():
    """Field order of the three structs the binding mirrors (a reordered header would silently shift every value)."""
    def fields(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith("uint64_t") and not decl.startswith("size_t") else decl.split(None, 1)[1]
            for n in names.split(","):
                out.append(re.sub(r"\[.*\]", "", n.strip().lstrip("*")))
        return out
    assert fields("sn_auto_state") == [f for f, _ in api.SnAutoState._fields_]
    assert fields("sn_refine_stats") == [f for f, _ in api.SnRefineStats._fields_]
    assert fields("sn_io_info") == [f for f, _ in api.SnIoInfo._fields_]
    assert fields("sn_config") == [f for f, _ in api.SnConfig._fields_]


# ---- the range check (SN_ERR_RANGE): a call whose fp16 storage overflowed reports residual_px = +inf ---------------------------
def test_a_flagged_residual_leaves_f16_and_never_comes_back(lib):
    inf = float("inf")
    s = _state(lib)
    assert lib.sn_auto_observe(C.byref(s), inf) == api.PREC_F16X3 and s.switches == 1
    assert s.running_px == 1e30                               # folded in as the cap, so that the mean can come back
    for _ in range(3 * CALM):
        assert lib.sn_auto_observe(C.byref(s), inf) == api.PREC_F16X3
    assert s.switches == 1 and s.calm == 0
    # one flagged call among calm ones resets the count like any call outside the band
    for _ in range(CALM - 1):
        lib.sn_auto_observe(C.byref(s), 0.1)
    assert lib.sn_auto_observe(C.byref(s), inf) == api.PREC_F16X3 and s.calm == 0
    for i in range(CALM):
        assert lib.sn_auto_observe(C.byref(s), 0.1) == (api.PREC_F16 if i == CALM - 1 else api.PREC_F16X3)
    assert s.running_px < 1e30


def test_the_range_error_is_declared_bound_and_distinct(lib):
    assert re.search(r"SN_ERR_RANGE\s*=\s*-8", HEADER) and api.SN_ERR_RANGE == -8
    assert "65504" in api.error_string(-8) and "SN_PREC_FP32" in api.error_string(-8)
    assert "65504" in HEADER and "Use SN_PREC_FP32 for such a model" in HEADER
    assert [f for f, _ in api.SnRefineStats._fields_][-2:] == ["nonfinite_px", "nonfinite_low_px"]
    assert C.sizeof(api.SnRefineStats) == 4 * 4 + 4 * 8 + 4 * 8 + 6 * 8 + 4 * 8 + 8
    e = api.StereoNetRangeError("sn_infer_batch", "detail", [0, 0, 7, 0], 3)
    assert isinstance(e, api.StereoNetError) and e.code == api.SN_ERR_RANGE
    assert e.nonfinite_px == [0, 0, 7, 0] and e.nonfinite_low_px == 3 and e.outputs is None and "65504" in str(e)
    assert api.F16_MAX == 65504.0


def _rec(residual, last, reruns, switches, check=(-1.0, -1.0), **extra):
    return {"residual_px": residual, "precision_last": last, "reruns": reruns, "switches": switches,
            "selfcheck_epe_px": check[0], "selfcheck_residual_px": check[1], **extra}


def test_replay_accepts_a_flagged_call_and_only_what_the_state_machine_does(lib):
    """truth_compare.replay on what a handle of the default precision reports when the range check fires"""
    import truth_compare as tc
    inf = float("inf")
    # first call flagged in F16 (no self-check is owed), repeated in F16X3 and flagged there too; then the handle stays
    flagged = [_rec(inf, "f16x3", 1, 1), _rec(inf, "f16x3", 1, 1), _rec(inf, "f16x3", 1, 1)]
    assert tc.replay(flagged, pure=lib) == []
    # the repeat is finite (only the fp16 tower overflowed): the record carries what was observed
    assert tc.replay([_rec(0.5, "f16x3", 1, 1, observed_px=inf), _rec(0.5, "f16x3", 1, 1)], pure=lib) == []
    # teeth: a flagged call that stayed in F16, one that was not repeated, one that calibrated on the flagged pair
    assert tc.replay([_rec(inf, "f16", 0, 0)], pure=lib)
    assert tc.replay([_rec(inf, "f16x3", 0, 1)], pure=lib)
    assert tc.replay([_rec(inf, "f16x3", 1, 1, check=(0.0, 0.3))], pure=lib)
    # a calm first call calibrates as before, a later flagged one switches at once
    ok = [_rec(0.3, "f16", 0, 0, check=(1e-4, 0.3)), _rec(inf, "f16x3", 1, 1, check=(1e-4, 0.3))]
    assert tc.replay(ok, pure=lib) == []
