"""Per-pixel confidence of the disparity map: the numpy twin of sn_infer_conf / sn_conf_mask (include/stereonet_hip.h).

The soft-argmin holds the whole matching distribution of a low-resolution pixel and reports its expectation `dhat`.  `low` is
the probability mass on the two cost planes that bracket that expectation: 1 for a single peak (or one shared by two
neighbouring planes, an honest sub-plane disparity), about the mass that happens to lie under the mean for two far-apart
peaks, 2 / Dl for a flat distribution.  `upsample` brings the plane to the map's size the way the refinement's disparity input
is upsampled (bilinear x16, half-pixel centres, edge clamp, factor 1 on the values), and `mask` applies a threshold in the wire
format of the other post-processing (lrcheck, dispfilter): a rejected pixel gets raw = 0, "no measurement".

`low` and `upsample` work in float64 (the kernels in fp32: csrc/sn_kernels.hpp softargmin_conf, csrc/sn_confidence.hpp); `mask`
is exact.
"""
from __future__ import annotations

import numpy as np

KEPT, INVALID_IN, LOW = 0, 1, 64      # SN_CONF_*; disjoint from the SN_LRC_* (1, 2, 4, 8) and SN_FLT_* (16, 32) bits
FACTOR = 16                           # full-resolution pixels per low-resolution pixel


def low(cost, disp_low) -> np.ndarray:
    """cost (Dl,hl,wl) or (n,Dl,hl,wl), disp_low (hl,wl) / (n,hl,wl) float32 = the soft-argmin's stored expectation ->
    conf_low float64 of disp_low's shape.  The bracket k = min(floor(dhat), Dl - 2) is taken from the GIVEN float32 disp_low,
    so a caller that passes a kernel's own disp_low judges the kernel's sum, not its rounding of the floor."""
    c = np.asarray(cost, np.float64)
    d = np.asarray(disp_low, np.float32)
    if c.ndim not in (3, 4) or d.shape != c.shape[:-3] + c.shape[-2:]:
        raise ValueError(f"low: cost of shape {c.shape} and disp_low of shape {d.shape}")
    Dl = c.shape[-3]
    if Dl == 1:
        return np.ones(d.shape, np.float64)
    m = (-c).max(-3, keepdims=True)
    e = np.exp(-c - m)
    se = e.sum(-3)
    k = np.minimum(np.floor(d).astype(np.int64), Dl - 2)
    k = np.clip(k, 0, Dl - 2)[..., None, :, :]           # (dhat lies in [0, Dl - 1]; the clip only guards a NaN input)
    e0 = np.take_along_axis(e, k, -3)
    e1 = np.take_along_axis(e, k + 1, -3)
    return ((e0 + e1)[..., 0, :, :]) / se


def upsample(conf_low, h: int, w: int) -> np.ndarray:
    """(hl,wl) or (n,hl,wl) -> float64 (..., h, w): bilinear x16, align_corners=False (half-pixel centres, edge clamp), cropped
    to h x w — torch.nn.functional.interpolate(scale_factor=16, mode="bilinear", align_corners=False)[..., :h, :w]."""
    a = np.asarray(conf_low, np.float64)
    if a.ndim not in (2, 3):
        raise ValueError(f"upsample: shape {a.shape} is not ([n,] hl, wl)")
    hl, wl = a.shape[-2:]
    if not (0 < h <= FACTOR * hl and 0 < w <= FACTOR * wl):
        raise ValueError(f"upsample: {w}x{h} does not fit {FACTOR} x {wl}x{hl}")

    def taps(n_out, n_low):
        s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) / FACTOR - 0.5, 0.0)
        i0 = np.floor(s).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_low - 1)
        return i0, i1, s - i0
    y0, y1, ly = taps(h, hl)
    x0, x1, lx = taps(w, wl)
    top = a[..., y0, :][..., :, x0] * (1.0 - lx) + a[..., y0, :][..., :, x1] * lx
    bot = a[..., y1, :][..., :, x0] * (1.0 - lx) + a[..., y1, :][..., :, x1] * lx
    return top * (1.0 - ly)[:, None] + bot * ly[:, None]


def mask(raw, conf, min_conf: float):
    """sn_conf_mask: int32 raw and float conf of one shape, (H,W) or (n,H,W) -> (out_raw int32, mask uint8, kept uint32 (n,)).
    raw <= 0 -> INVALID_IN; not (conf >= min_conf) -> LOW (a NaN confidence is rejected at every threshold); else kept."""
    if not (np.isfinite(min_conf) and 0.0 <= min_conf <= 1.0):
        raise ValueError("min_conf must be finite and in [0, 1]")
    r = np.ascontiguousarray(raw, np.int32)
    c = np.asarray(conf, np.float32)
    if r.shape != c.shape or r.ndim not in (2, 3):
        raise ValueError(f"raw of shape {r.shape} and conf of shape {c.shape}")
    with np.errstate(invalid="ignore"):
        ok = c >= np.float32(min_conf)
    m = np.where(r <= 0, INVALID_IN, np.where(ok, KEPT, LOW)).astype(np.uint8)
    out = np.where(m == KEPT, r, 0).astype(np.int32)
    kept = (m == KEPT).reshape(1 if r.ndim == 2 else r.shape[0], -1).sum(1).astype(np.uint32)
    return out, m, kept
