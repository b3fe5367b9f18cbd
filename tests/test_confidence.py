"""The confidence of the soft-argmin distribution as its numpy twin (hobot_stereonet_amd/confidence.py) — no GPU.  Known
answers of the low-resolution definition (include/stereonet_hip.h), the x16 upsample against torch's bilinear interpolation,
the mask rules at their edges, and the agreement of the Python binding with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, confidence, filelist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
BIG = 200.0      # a cost this far above the minimum has probability exp(-200): nothing in float64 sums


def _expectation(cost):
    """the soft-argmin's dhat of a (Dl, h, w) cost in float64, as the float32 the kernels store"""
    c = np.asarray(cost, np.float64)
    e = np.exp(-c - (-c).max(0, keepdims=True))
    return ((np.arange(c.shape[0])[:, None, None] * e).sum(0) / e.sum(0)).astype(np.float32)


def _cost(planes, Dl):
    """(Dl, 1, 1): cost 0 on `planes`, BIG elsewhere — equal mass on the given planes"""
    c = np.full((Dl, 1, 1), BIG)
    c[list(planes)] = 0.0
    return c


def test_header_and_binding_agree():
    enums = {k: int(v) for k, v in re.findall(r"\b(SN_CONF_[A-Z0-9_]+)\s*=\s*(\d+)", HEADER)}
    assert enums == {"SN_CONF_KEPT": 0, "SN_CONF_INVALID_IN": 1, "SN_CONF_LOW": 64}
    for name, value in enums.items():
        assert getattr(api, name) == value
    assert (confidence.KEPT, confidence.INVALID_IN, confidence.LOW) == (0, 1, 64)
    lrc_bits = {int(v) for v in re.findall(r"\bSN_LRC_(?!IN_)[A-Z_]+\s*=\s*(\d+)", HEADER)}
    flt_bits = {int(v) for v in re.findall(r"\bSN_FLT_(?!INVALID_IN)[A-Z_]+\s*=\s*(\d+)", HEADER)}
    assert lrc_bits == {0, 1, 2, 4, 8} and flt_bits == {16, 32}
    assert not any(confidence.LOW & b for b in lrc_bits | flt_bits)          # masks can be OR-ed
    body = re.search(r"typedef struct sn_conf_params \{(.*?)\} sn_conf_params;", HEADER, re.S).group(1)
    decls = [d.split() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert [(t, n) for t, n in decls] == [("float", "min_conf")]
    assert api.SnConfParams._fields_ == [("min_conf", C.c_float)] and C.sizeof(api.SnConfParams) == 4
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # 4: SN_ERR_RANGE and the range counts of sn_refine_stats; these structs are as in 3
    lib = api.load_library()
    for sym in ("sn_infer_conf", "sn_conf_mask"):
        assert re.search(rf"\bint {sym}\(", HEADER) and hasattr(lib, sym)
        assert getattr(lib, sym).restype is C.c_int
    assert len(lib.sn_infer_conf.argtypes) == 14 and len(lib.sn_conf_mask.argtypes) == 11
    for name in ("infer_conf", "infer_conf_device", "conf_mask", "conf_mask_device"):
        assert callable(getattr(api.StereoNetHIP, name))


@pytest.mark.parametrize("Dl", [2, 6, 16])
def test_one_hot_flat_and_neighbouring_planes(Dl):
    for k in range(Dl):                                                        # a single peak, wherever it sits
        c = _cost([k], Dl)
        assert confidence.low(c, _expectation(c))[0, 0] == pytest.approx(1.0, abs=1e-15)
    flat = np.zeros((Dl, 2, 3))
    got = confidence.low(flat, _expectation(flat))
    assert got.shape == (2, 3) and got.dtype == np.float64 and np.allclose(got, 2.0 / Dl, rtol=0, atol=1e-15)
    for k in range(Dl - 1):                                                    # a peak shared by planes k, k + 1
        c = _cost([k, k + 1], Dl)
        d = _expectation(c)
        assert d[0, 0] == np.float32(k + 0.5)
        assert confidence.low(c, d)[0, 0] == pytest.approx(1.0, abs=1e-15)


def test_single_plane_is_one():
    c = np.random.default_rng(0).normal(size=(2, 1, 3, 4))
    got = confidence.low(c, np.zeros((2, 3, 4), np.float32))
    assert got.shape == (2, 3, 4) and np.all(got == 1.0)


def test_two_far_peaks_and_the_last_bracket():
    c = _cost([0, 5], 6)                                                       # equal mass on planes 0 and Dl - 1
    d = _expectation(c)
    assert d[0, 0] == np.float32(2.5)                                          # the mean lies under neither peak
    assert confidence.low(c, d)[0, 0] == pytest.approx(0.0, abs=1e-80)
    assert confidence.low(c, np.float32([[0.0]]))[0, 0] == pytest.approx(0.5, abs=1e-15)     # bracket (0, 1) holds one of them
    # dhat == Dl - 1 exactly: k = min(5, Dl - 2) = 4, the bracket (Dl - 2, Dl - 1)
    assert confidence.low(c, np.float32([[5.0]]))[0, 0] == pytest.approx(0.5, abs=1e-15)
    c = np.zeros((6, 1, 1))
    c[:, 0, 0] = [BIG, BIG, BIG, BIG, np.log(3.0), 0.0]                        # p4 = 1/4, p5 = 3/4
    assert confidence.low(c, np.float32([[5.0]]))[0, 0] == pytest.approx(1.0, abs=1e-15)
    assert confidence.low(c, np.float32([[3.0]]))[0, 0] == pytest.approx(0.25, abs=1e-15)    # bracket (3, 4)
    # batched input, the bracket per pixel from the given disp_low
    cb = np.stack([_cost([1], 4), _cost([1, 3], 4)])
    got = confidence.low(cb, np.float32([[[1.0]], [[2.0]]]))
    assert got.shape == (2, 1, 1) and got[0, 0, 0] == pytest.approx(1.0) and got[1, 0, 0] == pytest.approx(0.5)
    with pytest.raises(ValueError):
        confidence.low(np.zeros((4, 2, 2)), np.zeros((3, 2), np.float32))


def test_upsample_is_torch_bilinear():
    import torch
    rng = np.random.default_rng(1)
    low = rng.random((2, 3, 3))
    h, w = 33, 47
    want = torch.nn.functional.interpolate(torch.from_numpy(low)[:, None], scale_factor=16, mode="bilinear",
                                           align_corners=False)[:, 0, :h, :w].numpy()
    got = confidence.upsample(low, h, w)
    assert got.dtype == np.float64 and got.shape == (2, h, w)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(confidence.upsample(low[0], h, w) - want[0]).max() <= 1e-12
    assert np.all(confidence.upsample(np.full((1, 1), 0.25), 16, 16) == 0.25)          # a 1x1 grid: every tap is the one value
    with pytest.raises(ValueError):
        confidence.upsample(low, 49, 47)


def test_mask_rules():
    raw = np.array([[-7, 0, 5, 5, 5, 5, 2 ** 31 - 1]], np.int32)
    conf = np.array([[1.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, 0.75, 0.0]], np.float32)
    out, mask, kept = confidence.mask(raw, conf, 0.5)
    assert mask.dtype == np.uint8 and mask.tolist() == [[1, 1, 0, 64, 64, 0, 64]]     # the threshold exactly met is kept
    assert out.dtype == np.int32 and out.tolist() == [[0, 0, 5, 0, 0, 5, 0]]
    assert kept.dtype == np.uint32 and kept.tolist() == [2]
    out, mask, kept = confidence.mask(raw, conf, 0.0)                                  # 0 rejects only NaN (and raw <= 0)
    assert mask.tolist() == [[1, 1, 0, 0, 64, 0, 0]] and kept.tolist() == [4]
    out, mask, kept = confidence.mask(raw, conf, 1.0)
    assert mask.tolist() == [[1, 1, 64, 64, 64, 64, 64]] and kept.tolist() == [0]
    out, mask, kept = confidence.mask(np.stack([raw, raw]), np.stack([conf, np.ones_like(conf)]), 0.5)
    assert kept.tolist() == [2, 5] and mask.shape == (2, 1, 7)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            confidence.mask(raw, conf, bad)
    with pytest.raises(ValueError):
        confidence.mask(raw, conf[:, :-1], 0.5)


@pytest.mark.parametrize("value", ["-0.1", "1.5", "nan", "abc", "inf", "0.5,0.5"])
def test_filelist_rejects_bad_conf(value, tmp_path, capsys):
    with pytest.raises(SystemExit):
        filelist.main(["--model", "m", "--left", "l", "--right", "r", "--conf", value])
    capsys.readouterr()
