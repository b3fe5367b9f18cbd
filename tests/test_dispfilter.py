"""Speckle removal and hole filling as the numpy twin (hobot_stereonet_amd/dispfilter.py) — no GPU.  The twin against
implementations written from the contract in include/stereonet_hip.h (the flood fill and the per-pixel scalar fill loop of
tests/golden/plain_refs.py, scipy.ndimage.label), known answers at every boundary of the contract, and the agreement of the Python binding with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, dispfilter
from hobot_stereonet_amd.dispfilter import FILLED, INVALID_IN, SPECKLE
from plain_refs import filter_independent as _independent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
S = float(dispfilter.wire_scale())
IMAX = 2 ** 31 - 1


def _px(dq):
    """a speckle_diff_px whose diff_units is exactly dq: the middle of the interval the floor maps to dq"""
    d = (dq + 0.5) * S
    assert dispfilter.diff_units(d) == dq
    return d


def test_twin_equals_flood_fill_and_scalar_fill_on_random_maps():
    rng = np.random.default_rng(11)
    shapes = [(1, 1), (1, 37), (29, 1), (40, 70), (17, 64), (16, 65), (33, 5)] + \
             [(int(rng.integers(2, 41)), int(rng.integers(2, 71))) for _ in range(13)]
    seen = set()
    for i, (H, W) in enumerate(shapes):
        raw = rng.integers(1, 7, (H, W)).astype(np.int32)
        raw[rng.random((H, W)) < 0.3] = 0
        raw[rng.random((H, W)) < 0.05] = -int(rng.integers(1, 9))
        dq, max_px, fill_max = i % 4, min(int(rng.integers(1, 9)), H * W), int(rng.integers(1, 6))
        for mp, fm in ((max_px, 0), (0, fill_max), (max_px, fill_max)):
            out, mask, counts = dispfilter.reference(raw, mp, _px(dq), fm)
            w_out, w_mask = _independent(raw, mp, dq, fm)
            assert np.array_equal(out, w_out) and np.array_equal(mask, w_mask), (H, W, dq, mp, fm)
            assert counts.tolist() == [[int((w_out > 0).sum()), int((w_mask & SPECKLE != 0).sum()), int((w_mask & FILLED != 0).sum())]]
            assert np.array_equal(out > 0, (mask == 0) | (mask & FILLED != 0))
            seen |= set(np.unique(mask).tolist())
    assert seen == {0, 1, 16, 33, 48}
    # a batch is its maps one by one
    stack = rng.integers(-1, 5, (3, 9, 20)).astype(np.int32)
    o3, m3, c3 = dispfilter.reference(stack, 3, _px(1), 2)
    for k in range(3):
        o, m, c = dispfilter.reference(stack[k], 3, _px(1), 2)
        assert np.array_equal(o3[k], o) and np.array_equal(m3[k], m) and c3[k].tolist() == c[0].tolist()


def test_component_sizes_equal_scipy_label_at_full_width():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    W, H = 1242, 375
    raw = rng.integers(1, IMAX, (H, W), dtype=np.int64).astype(np.int32)
    raw[rng.random((H, W)) < 0.42] = 0                     # near the percolation threshold: components of every size
    dq = dispfilter.diff_units(3.0e6)
    assert dq >= IMAX                                      # every valid neighbour pair links
    lab = dispfilter.label(raw, dq)
    ref, ncomp = ndimage.label(raw > 0)                    # 4-connectivity is scipy's default structure
    sizes = np.bincount(ref.ravel())
    valid = raw > 0
    assert np.array_equal(np.bincount(lab.ravel(), minlength=raw.size)[lab][valid], sizes[ref][valid])
    assert len(np.unique(lab[valid])) == ncomp
    first = np.full(ncomp + 1, raw.size, np.int64)         # the label is the component's smallest pixel index
    np.minimum.at(first, ref.ravel(), np.arange(raw.size))
    assert np.array_equal(lab[valid], first[ref][valid])
    for max_px in (1, 50, 5000):
        out, mask, counts = dispfilter.reference(raw, max_px, 3.0e6, 0)
        assert np.array_equal(mask == SPECKLE, valid & (sizes[ref] <= max_px))
        assert np.array_equal(out, np.where(valid & (sizes[ref] > max_px), raw, 0))


def test_speckle_known_answers():
    z = np.zeros((9, 12), np.int32)
    # exactly max pixels: removed; max + 1: survives
    a = z.copy()
    a[1, 1:5] = 100                      # 4 pixels
    a[4:6, 2:4] = 100                    # 4 pixels, a square
    a[7, 1:6] = 100                      # 5 pixels
    out, mask, counts = dispfilter.reference(a, 4, _px(0), 0)
    assert np.all(out[1] == 0) and np.all(out[4:6] == 0) and np.array_equal(out[7], a[7])
    assert np.all(mask[1, 1:5] == SPECKLE) and np.all(mask[4:6, 2:4] == SPECKLE) and np.all(mask[7, 1:6] == 0)
    assert counts.tolist() == [[5, 8, 0]]
    # diagonal neighbours are not connected
    d = z.copy()
    d[2, 2] = d[3, 3] = d[4, 4] = 7
    assert dispfilter.reference(d, 2, _px(5), 0)[2].tolist() == [[0, 3, 0]]
    # two plateaus differing by dq are one component, by dq + 1 two
    for dq in (0, 1, 1999, dispfilter.diff_units(1.0)):
        for step, removed in ((dq, 0), (dq + 1, 6)):
            p = z.copy()
            p[3, 0:6] = 5000
            p[3, 6:12] = 5000 + step     # 6 + 6 pixels in a row
            for arr in (p, np.ascontiguousarray(p.T)):
                o, m, c = dispfilter.reference(arr, 6, _px(dq), 0)
                assert c[0, 1] == 2 * removed and c[0, 0] == 12 - 2 * removed, (dq, step)
    # INT32_MAX beside 1: the difference is taken in 64 bits, and 2^31 - 2 > dq
    e = z.copy()
    e[0, 0:2] = [IMAX, 1]
    e[5:7, 5] = [1, IMAX]
    o, m, c = dispfilter.reference(e, 1, 1.0, 0)
    assert c.tolist() == [[0, 4, 0]]
    o, m, c = dispfilter.reference(e, 1, 3.0e6, 0)          # dq covers the whole int32 range: pairs of two
    assert c.tolist() == [[4, 0, 0]] and np.array_equal(o, e)
    # a negative input yields 0 with mask 1, in either stage
    n = z.copy()
    n[0, 0] = -7
    n[0, 1] = -IMAX - 1
    for mp, fm in ((3, 0), (0, 3)):
        o, m, c = dispfilter.reference(n, mp, 1.0, fm)
        assert not o.any() and np.all(m == INVALID_IN) and c.tolist() == [[0, 0, 0]]


def test_fill_known_answers():
    def run(row, fm, mp=0):
        o, m, c = dispfilter.reference(np.asarray([row], np.int32), mp, 1.0, fm)
        return o[0].tolist(), m[0].tolist(), c[0].tolist()

    # a gap of fill_max is filled, one of fill_max + 1 is not; min picks the background side
    assert run([9, 0, 0, 0, 5, 0, 0, 0, 0, 7], 3) == ([9, 5, 5, 5, 5, 0, 0, 0, 0, 7], [0, 33, 33, 33, 0, 1, 1, 1, 1, 0], [6, 0, 3])
    assert run([9, 0, 0, 0, 5, 0, 0, 0, 0, 7], 4)[0] == [9, 5, 5, 5, 5, 5, 5, 5, 5, 7]
    assert run([5, 0, 9], 1)[0] == [5, 5, 9] and run([9, 0, 5], 1)[0] == [9, 5, 5]
    # gaps at the borders take their one neighbour; their length counts from the border
    assert run([0, 0, 4, 8, 0, 0, 0], 3) == ([4, 4, 4, 8, 8, 8, 8], [33, 33, 0, 0, 33, 33, 33], [7, 0, 5])
    assert run([0, 0, 4, 8, 0, 0, 0], 2) == ([4, 4, 4, 8, 0, 0, 0], [33, 33, 0, 0, 1, 1, 1], [4, 0, 2])
    # a row without valid pixels is untouched, whatever fill_max
    assert run([0, -3, 0, 0], 100) == ([0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0])
    # negatives are holes like zeros
    assert run([6, -1, 0, 6], 2)[:2] == ([6, 6, 6, 6], [0, 33, 33, 0])
    # a filled pixel is never a source: the middle gap is bounded by 3 and 8, not by anything filled
    assert run([3, 0, 8, 0, 0, 0, 2], 1) == ([3, 3, 8, 0, 0, 0, 2], [0, 33, 0, 1, 1, 1, 0], [4, 0, 1])
    # a removed speckle inside a short gap ends as 48 with the neighbours' value: the gap is measured on the stage-1 map
    big = np.zeros((4, 12), np.int32)
    big[:, 0:4] = 50
    big[:, 8:12] = 40
    big[1, 5] = 900                               # one pixel, unlike everything around it
    big[2, 4] = 50                                # grows the left plateau: no speckle
    o, m, c = dispfilter.reference(big, 2, _px(3), 4)
    assert o[1].tolist() == [50] * 4 + [40] * 8 and m[1].tolist() == [0] * 4 + [33, 48, 33, 33] + [0] * 4
    assert o[2].tolist() == [50] * 5 + [40] * 7 and c.tolist() == [[48, 1, 15]]
    o, m, c = dispfilter.reference(big, 2, _px(3), 3)          # the same gap is 4 wide once the speckle is gone: too wide
    assert o[1].tolist() == [50] * 4 + [0] * 4 + [40] * 4 and m[1, 5] == SPECKLE and o[2].tolist() == [50] * 5 + [40] * 7
    o, m, c = dispfilter.reference(big, 0, _px(3), 3)          # without stage 1 the speckle splits the gap and is a source
    assert o[1].tolist() == [50] * 5 + [900] + [40] * 6


def test_counts_equal_the_masks_bit_counts_and_arguments_are_checked():
    rng = np.random.default_rng(8)
    raw = rng.integers(1, 4, (2, 31, 45)).astype(np.int32) * 1000
    raw[rng.random(raw.shape) < 0.35] = 0
    out, mask, counts = dispfilter.reference(raw, 5, _px(10), 3)
    assert counts.shape == (2, 3) and counts.dtype == np.uint32 and out.dtype == np.int32 and mask.dtype == np.uint8
    for k in range(2):
        assert counts[k].tolist() == [int((out[k] > 0).sum()), int((mask[k] & SPECKLE != 0).sum()), int((mask[k] & FILLED != 0).sum())]
    assert counts[:, 1].min() > 0 and counts[:, 2].min() > 0
    assert dispfilter.diff_units(0.0) == 0 and dispfilter.diff_units(1.0) == int(np.floor(np.float32(1.0) / np.float32(S)))
    assert dispfilter.diff_units(3.0e38) == 2 ** 32
    for bad in ((0, 1.0, 0), (-1, 1.0, 1), (31 * 45 + 1, 1.0, 0), (1, -0.5, 0), (1, float("nan"), 0), (1, float("inf"), 0),
                (0, 1.0, -1)):
        with pytest.raises(ValueError):
            dispfilter.reference(raw, *bad)
    with pytest.raises(ValueError):
        dispfilter.reference(np.zeros(5, np.int32), 1, 1.0, 0)
    assert dispfilter.reference(raw, 31 * 45, 1.0, 0)[2][:, 0].tolist() == [0, 0]      # H*W itself is allowed: everything goes


def test_filter_binding_agrees_with_the_header():
    enums = {k: int(v) for k, v in re.findall(r"\b(SN_FLT_[A-Z0-9_]+)\s*=\s*(\d+)", HEADER)}
    assert enums == {"SN_FLT_INVALID_IN": 1, "SN_FLT_SPECKLE": 16, "SN_FLT_FILLED": 32}
    for name, value in enums.items():
        assert getattr(api, name) == value, name
    assert (dispfilter.INVALID_IN, dispfilter.SPECKLE, dispfilter.FILLED) == (1, 16, 32)
    body = re.search(r"typedef struct sn_filter_params \{(.*?)\} sn_filter_params;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    ctype = {"float": C.c_float, "int": C.c_int}
    assert [(name, ctype[t]) for t, name in decls] == list(api.SnFilterParams._fields_)
    assert C.sizeof(api.SnFilterParams) == 12
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # 4: SN_ERR_RANGE and the range counts of sn_refine_stats; these structs are as in 3
    proto = re.search(r"\bint sn_filter_raw\((.*?)\);", HEADER, re.S).group(1)
    params = [" ".join(t.split()) for t in proto.split(",")]
    assert params == ["sn_handle *h", "int n", "const int32_t *raw", "const sn_filter_params *p", "int32_t *out_raw",
                      "float *disp_inout", "uint8_t *mask", "uint32_t *counts", "int mem", "void *stream"]
    lib = api.load_library()
    assert hasattr(lib, "sn_filter_raw") and lib.sn_filter_raw.restype is C.c_int
    at = lib.sn_filter_raw.argtypes
    assert len(at) == len(params)
    assert at[1] is C.c_int and at[8] is C.c_int and at[3] is C.POINTER(api.SnFilterParams)
    assert all(at[i] is C.c_void_p for i in (0, 2, 4, 5, 6, 7, 9))
    assert dispfilter.OUT_SCALE == pytest.approx(float(re.search(r"float out_scale;\s*/\*\s*([0-9.e-]+)", HEADER).group(1)))
    assert callable(api.StereoNetHIP.filter_raw) and callable(api.StereoNetHIP.filter_raw_device)


@pytest.mark.parametrize("flag,value", [("--speckle", "0"), ("--speckle", "-5"), ("--speckle", "abc"), ("--speckle", "10,-1"),
                                        ("--speckle", "10,nan"), ("--speckle", "10,1,2"), ("--speckle", "2.5"),
                                        ("--fill", "0"), ("--fill", "-1"), ("--fill", "x"), ("--fill", "1.5"), ("--fill", "3,4")])
def test_filelist_rejects_bad_filter_arguments_before_any_work(flag, value, capsys):
    from hobot_stereonet_amd import filelist
    with pytest.raises(SystemExit):
        filelist.main(["--model", "none.snw", "--left", "none.list", "--right", "none.list", flag, value])
    assert f"{flag} takes MAX_PX" in capsys.readouterr().err
