"""Guided weighted-median smoothing of int32 disparity maps: the numpy twin of sn_smooth_raw (include/stereonet_hip.h), bit for
bit.

The filter (dispfilter.py) fills every row on its own, the left-right check lets well-connected outliers through and the
refinement leaves sub-pixel noise.  A median over a small window removes all three; weighting every window pixel by how close
its luma is to the centre's keeps the median from rounding corners and thin structures: across a luma edge the weights fall to
(almost) nothing, so each side is smoothed with its own pixels.  The weights are a 256-entry integer table (`weight_table`), the
median is the LOWER weighted median — the smallest participating value whose cumulative weight reaches half the total — so
the result depends on no traversal or tie order and the kernel (csrc/sn_smooth.hpp) has nothing to round differently.

`reference` is vectorised over the window offsets: every offset contributes one column of (value << 9 | weight) keys per
pixel, the keys are sorted per pixel, and the median is the first key whose running weight reaches half the total.
"""
from __future__ import annotations

import numpy as np

from .lrcheck import OUT_SCALE, wire_scale

INVALID_IN, CHANGED = 1, 128                 # SN_SMOOTH_* bits; 0 = a measurement the smoother left as it was
BITS = {INVALID_IN: "invalid_in", CHANGED: "changed"}
GUIDE_NV12, GUIDE_TENSOR = 0, 1              # SN_GUIDE_*


def weight_table(sigma_luma: int) -> np.ndarray:
    """T[0..255] of the contract as int32: all ones for sigma_luma == 0, else (256 s^2) // (s^2 + j^2)."""
    s = int(sigma_luma)
    if not 0 <= s <= 255:
        raise ValueError("sigma_luma must lie in 0..255")
    if s == 0:
        return np.ones(256, np.int32)
    j = np.arange(256, dtype=np.int64)
    return ((256 * s * s) // (s * s + j * j)).astype(np.int32)


def luma_from_tensor(x: np.ndarray) -> np.ndarray:
    """SN_GUIDE_TENSOR: the int8 model input (6,H,W) or (n,6,H,W) -> uint8 luma (H,W) or (n,H,W) = channel 0 with bit 7 flipped."""
    a = np.asarray(x)
    if a.dtype != np.int8 or a.ndim not in (3, 4) or a.shape[-3] != 6:
        raise ValueError(f"an int8 model input ([n,] 6, H, W), not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a[..., 0, :, :]).view(np.uint8) ^ np.uint8(0x80)


def luma_from_nv12(buf: np.ndarray, w: int, h: int, pitch: int = 0, n: int = 1) -> np.ndarray:
    """SN_GUIDE_NV12: n frames of pitch * (h + ceil(h/2)) bytes (pitch 0 = w) -> uint8 luma (n,h,w), the first w bytes of the
    first h rows of every frame (the left eye of a side-by-side frame when pitch = 2w)."""
    pitch = pitch or w
    frame = pitch * (h + (h + 1) // 2)
    b = np.asarray(buf, np.uint8).reshape(-1)
    if pitch < w or b.size < (n - 1) * frame + pitch * (h - 1) + w:
        raise ValueError(f"{b.size} bytes are not {n} NV12 frames of pitch {pitch}")
    out = np.empty((n, h, w), np.uint8)
    for k in range(n):
        rows = np.lib.stride_tricks.as_strided(b[k * frame:], (h, w), (pitch, 1), writeable=False)
        out[k] = rows
    return out


def _one(raw: np.ndarray, luma, radius: int, T: np.ndarray, min_valid: int):
    H, W = raw.shape
    D = 2 * radius + 1
    pad = np.zeros((H + 2 * radius, W + 2 * radius), np.int64)       # outside the image: no measurement, never a participant
    pad[radius:-radius, radius:-radius] = np.maximum(raw, 0)
    if luma is not None:
        lpad = np.zeros(pad.shape, np.int32)
        lpad[radius:-radius, radius:-radius] = luma
        lc = lpad[radius:-radius, radius:-radius]
    keys = np.empty((H, W, D * D), np.int64)
    measured = np.zeros((H, W), np.int32)
    none = np.int64(1) << 40                                         # sorts after every participant, weight bits 0
    for dy in range(D):
        for dx in range(D):
            q = pad[dy:dy + H, dx:dx + W]
            ok = q > 0
            measured += ok
            wq = ok.astype(np.int64) if luma is None else np.where(ok, T[np.abs(lpad[dy:dy + H, dx:dx + W] - lc)], 0).astype(np.int64)
            keys[:, :, dy * D + dx] = np.where(wq > 0, (q << 9) | wq, none)
    keys.sort(axis=-1)
    cum = np.cumsum(keys & 511, axis=-1)
    wt = cum[..., -1]
    first = np.argmax(2 * cum >= wt[..., None], axis=-1)             # the first key whose running weight reaches half
    m = np.take_along_axis(keys, first[..., None], -1)[..., 0] >> 9
    centre = pad[radius:-radius, radius:-radius]
    fill = (min_valid > 0) & (measured >= min_valid) & (wt > 0)
    out = np.where(centre > 0, m, np.where(fill, m, 0))
    mask = np.where(raw <= 0, INVALID_IN, 0) | np.where(out != centre, CHANGED, 0)
    return out.astype(np.int32), mask.astype(np.uint8)


def reference(raw, luma=None, radius: int = 2, sigma_luma: int = 12, min_valid: int = 0, out_scale: float = OUT_SCALE):
    """sn_smooth_raw: int32 (H,W) or (n,H,W) and the uint8 luma of the same shape (None allowed for sigma_luma == 0) ->
    (out int32, mask uint8, counts uint32 (n,3) = {valid, smoothed measurements, filled pixels}).  out_scale only takes part in
    the float map (`expected_disp`): the integer result does not depend on it."""
    r = np.ascontiguousarray(raw, np.int32)
    if r.ndim not in (2, 3):
        raise ValueError(f"maps of shape {r.shape}")
    single = r.ndim == 2
    if single:
        r = r[None]
    radius, sigma_luma, min_valid = int(radius), int(sigma_luma), int(min_valid)
    if radius not in (1, 2, 3) or not 0 <= min_valid <= (2 * radius + 1) ** 2:
        raise ValueError("radius must be 1, 2 or 3 and min_valid lie in 0..(2*radius+1)^2")
    T = weight_table(sigma_luma)
    y = None
    if sigma_luma > 0:
        if luma is None:
            raise ValueError("sigma_luma > 0 needs the luma")
        y = np.asarray(luma)
        if y.dtype != np.uint8 or y.shape != np.shape(raw):
            raise ValueError(f"luma must be uint8 of the maps' shape {np.shape(raw)}, not {y.dtype} {y.shape}")
        y = y.reshape(r.shape)
    out, mask = np.empty_like(r), np.empty(r.shape, np.uint8)
    for k in range(r.shape[0]):
        out[k], mask[k] = _one(r[k], None if y is None else y[k], radius, T, min_valid)
    ch = mask & CHANGED != 0
    inv = mask & INVALID_IN != 0
    n = r.shape[0]
    counts = np.stack([(out > 0).reshape(n, -1).sum(1), (ch & ~inv).reshape(n, -1).sum(1), (ch & inv).reshape(n, -1).sum(1)],
                      1).astype(np.uint32)
    if single:
        return out[0], mask[0], counts
    return out, mask, counts


def expected_disp(disp0: np.ndarray, out: np.ndarray, mask: np.ndarray, out_scale: float = OUT_SCALE) -> np.ndarray:
    """disp_inout after the call: (float)result * S (0.0 at a result of 0) where SN_SMOOTH_CHANGED is set, disp0's bits elsewhere."""
    val = np.where(out > 0, out.astype(np.float32) * wire_scale(out_scale), np.float32(0)).astype(np.float32)
    return np.where(mask & CHANGED != 0, val.view(np.uint32), np.ascontiguousarray(disp0, np.float32).view(np.uint32)).view(np.float32)


def noisy_scene(w: int, h: int, seed: int = 0, out_scale: float = OUT_SCALE):
    """A piecewise-smooth test scene -> (raw int32 (h,w), luma uint8 (h,w), truth float64 px): a slanted background and a
    foreground slab whose luma edge lies on its disparity edge, 0.3 px of noise, 2 % outliers of 8 px, 5 % single holes and
    the occlusion strip left of the slab."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = 10.0 + 0.03 * x * (96.0 / w) + 0.02 * y
    fg = (x >= int(0.3 * w)) & (x < int(0.65 * w)) & (y >= int(0.25 * h)) & (y < int(0.8 * h))
    truth[fg] += 12.0
    luma = 70.0 + 25.0 * np.sin(x / 9.0) * np.cos(y / 7.0)
    luma[fg] = 190.0 + 15.0 * np.sin(y[fg] / 5.0)
    luma = np.clip(np.rint(luma + rng.normal(0.0, 2.0, (h, w))), 0, 255).astype(np.uint8)
    d = truth + rng.normal(0.0, 0.3, (h, w))
    outl = rng.random((h, w)) < 0.02
    d[outl] += np.where(rng.random(int(outl.sum())) < 0.5, 8.0, -8.0)
    raw = np.maximum(np.rint(d / float(wire_scale(out_scale))), 1).astype(np.int32)
    raw[rng.random((h, w)) < 0.05] = 0
    strip = max(4, w // 40)
    raw[int(0.25 * h):int(0.8 * h), int(0.3 * w) - strip:int(0.3 * w)] = 0
    return raw, luma, truth
