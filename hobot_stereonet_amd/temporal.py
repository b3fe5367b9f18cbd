"""Temporal filter of int32 disparity streams: the numpy twin of sn_temporal_push (include/stereonet_hip.h), bit for bit.

Every other stage of the chain treats a map on its own; this one keeps, per stream and pixel, the last filtered value P, the
validity history Hs of the last eight inputs and the last luma Yp.  A measurement near P is blended with it (an exponential
average with weight alpha / 256), one far from it replaces it (JUMP), a pixel without a measurement keeps P while enough of
its recent inputs held one (HELD), and a luma change above luma_delta says that the scene moved: no blending, no holding.
All of it is integer arithmetic, so the kernel (csrc/sn_temporal.hpp) has nothing to round differently.

`TemporalState.push` filters one frame, vectorised over the pixels; `reference` runs a whole call — n maps, each the next
frame of the stream `stream_of` names — and is what sn_temporal_push must equal.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .dispfilter import diff_units
from .lrcheck import OUT_SCALE, wire_scale

INVALID_IN, BLENDED, HELD, MOVED, JUMP = 1, 2, 4, 8, 16      # SN_TMP_*: a plane of its own, never OR-ed with the chain's mask
BITS = {INVALID_IN: "invalid_in", BLENDED: "blended", HELD: "held", MOVED: "moved", JUMP: "jump"}
MASK_VALUES = (0, 1, 2, 5, 8, 9, 16)


class Params(NamedTuple):
    """sn_temporal_params"""
    alpha: int = 64
    delta_px: float = 0.5
    persist: int = 2
    luma_delta: int = 24


def check_params(p) -> Params:
    p = Params(*p)
    if not 1 <= int(p.alpha) <= 256:
        raise ValueError("alpha must lie in 1..256")
    if not (np.isfinite(p.delta_px) and p.delta_px >= 0):
        raise ValueError("delta_px must be finite and >= 0")
    if not 0 <= int(p.persist) <= 8:
        raise ValueError("persist must lie in 0..8")
    if not 0 <= int(p.luma_delta) <= 255:
        raise ValueError("luma_delta must lie in 0..255")
    return Params(int(p.alpha), float(p.delta_px), int(p.persist), int(p.luma_delta))


def delta_for(q: int, out_scale: float = OUT_SCALE) -> float:
    """A delta_px that the contract turns into exactly q raw units (0 <= q < 2^24)."""
    d = float(np.float32((q + 0.5) * float(wire_scale(out_scale))))
    assert diff_units(d, out_scale) == q
    return d


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


class TemporalState:
    """The state of ONE stream: P (int64 here, always within int32), Hs, Yp per pixel, and whether it has seen a frame."""

    def __init__(self, h: int, w: int):
        self.shape = (h, w)
        self.reset()

    def reset(self):
        self.P = np.zeros(self.shape, np.int64)
        self.Hs = np.zeros(self.shape, np.int64)
        self.Yp = np.zeros(self.shape, np.int64)
        self.seen = False

    def push(self, raw: np.ndarray, luma: Optional[np.ndarray], alpha: int, q: int, persist: int, luma_delta: int):
        """One frame: int32 (H,W) [+ uint8 luma (H,W)] -> (out int32, mask uint8); q = delta_px in raw units."""
        r = np.maximum(np.asarray(raw).astype(np.int64), 0)
        if r.shape != self.shape:
            raise ValueError(f"a map of shape {r.shape}, the state is {self.shape}")
        P, Hs = self.P, self.Hs
        if luma_delta > 0:
            y = np.asarray(luma).astype(np.int64)
            moved = (np.abs(y - self.Yp) > luma_delta) if self.seen else np.zeros(self.shape, bool)
        else:
            moved = np.zeros(self.shape, bool)
        valid, had = r > 0, P > 0
        blend = valid & had & ~moved & (np.abs(r - P) <= q)
        mixed = (alpha * r + (256 - alpha) * P + 128) >> 8
        hold = ~valid & (persist > 0) & had & ~moved & (_POP[Hs] >= persist)
        out = np.where(valid, np.where(blend, mixed, r), np.where(hold, P, 0))
        mask = np.where(valid, 0, INVALID_IN)
        mask |= np.where(blend & (out != r), BLENDED, 0)
        mask |= np.where(valid & ~blend & had, np.where(moved, MOVED, JUMP), 0)
        mask |= np.where(hold, HELD, 0)
        drop = ~valid & ~hold & had & moved
        mask |= np.where(drop, MOVED, 0)
        Pn = np.where(valid, out, np.where(drop, 0, P))
        Hn = ((Hs << 1) | valid) & 255
        self.P = np.where(Hn == 0, 0, Pn)
        self.Hs = Hn
        if luma_delta > 0:
            self.Yp = y
        self.seen = True
        return out.astype(np.int32), mask.astype(np.uint8)


def counts_of(out: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """counts [n][4] of the contract from (n,H,W) results: {out > 0, BLENDED, HELD, MOVED or JUMP}"""
    n = out.shape[0]
    cols = [out > 0, mask & BLENDED != 0, mask & HELD != 0, mask & (MOVED | JUMP) != 0]
    return np.stack([c.reshape(n, -1).sum(1) for c in cols], 1).astype(np.uint32)


def reference(raw, luma=None, params=Params(), stream_of=None, states=None, out_scale: float = OUT_SCALE):
    """sn_temporal_push: raw int32 (n,H,W), luma uint8 (n,H,W) (None allowed for luma_delta == 0), params = (alpha, delta_px,
    persist, luma_delta), stream_of = n stream ids (None: one clip, stream 0) -> (out int32, mask uint8, counts uint32 (n,4)).
    states: a dict {id: TemporalState} that carries the streams across calls (updated in place; missing ids start fresh)."""
    p = check_params(params)
    r = np.ascontiguousarray(raw, np.int32)
    if r.ndim != 3:
        raise ValueError(f"maps of shape {r.shape}, not (n, H, W)")
    n = r.shape[0]
    ids = [0] * n if stream_of is None else [int(s) for s in stream_of]
    if len(ids) != n or min(ids) < 0:
        raise ValueError("stream_of must name one stream id >= 0 per map")
    y = None
    if p.luma_delta > 0:
        if luma is None:
            raise ValueError("luma_delta > 0 needs the luma")
        y = np.asarray(luma)
        if y.dtype != np.uint8 or y.shape != r.shape:
            raise ValueError(f"luma must be uint8 of the maps' shape {r.shape}, not {y.dtype} {y.shape}")
    q = diff_units(p.delta_px, out_scale)
    states = {} if states is None else states
    out, mask = np.empty_like(r), np.empty(r.shape, np.uint8)
    for k in range(n):
        st = states.setdefault(ids[k], TemporalState(*r.shape[1:]))
        out[k], mask[k] = st.push(r[k], None if y is None else y[k], p.alpha, q, p.persist, p.luma_delta)
    return out, mask, counts_of(out, mask)


def expected_disp(disp0: np.ndarray, raw: np.ndarray, out: np.ndarray, out_scale: float = OUT_SCALE) -> np.ndarray:
    """disp_inout after the call: (float)out * S exactly where out != max(raw, 0), disp0's bits elsewhere."""
    val = (out.astype(np.float32) * wire_scale(out_scale)).astype(np.float32)
    changed = out != np.maximum(np.asarray(raw, np.int32), 0)
    return np.where(changed, val.view(np.uint32), np.ascontiguousarray(disp0, np.float32).view(np.uint32)).view(np.float32)


def noisy_sequence(w: int, h: int, frames: int = 12, seed: int = 0, out_scale: float = OUT_SCALE):
    """A test clip -> (raw int32 (T,h,w), luma uint8 (T,h,w), truth float64 (T,h,w) in raw units): a static ramp background
    with +-150 raw units of noise per frame, 8 % dropouts, 1 % negatives and 1 % outliers of +5000, and a bright square (its own,
    nearer disparity) that moves 3 px per frame.  Every value a setting's mask can take occurs in it (tests/test_temporal.py)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ramp = 20000.0 + 40.0 * x * (96.0 / w) + 25.0 * y
    texture = 70.0 + 20.0 * np.sin(x / 9.0) * np.cos(y / 7.0)
    side = max(8, h // 4)
    raw = np.empty((frames, h, w), np.int32)
    luma = np.empty((frames, h, w), np.uint8)
    truth = np.empty((frames, h, w), np.float64)
    for t in range(frames):
        x0, y0 = w // 8 + 3 * t, h // 3
        sq = (x >= x0) & (x < x0 + side) & (y >= y0) & (y < y0 + side)
        truth[t] = np.where(sq, ramp + 12000.0, ramp)
        luma[t] = np.clip(np.rint(np.where(sq, 210.0, texture) + rng.integers(-2, 3, (h, w))), 0, 255).astype(np.uint8)
        v = np.rint(truth[t]).astype(np.int64) + rng.integers(-150, 151, (h, w))
        u = rng.random((h, w))
        v = np.where(u < 0.01, v + 5000, v)
        v = np.where((u >= 0.01) & (u < 0.09), 0, v)
        v = np.where((u >= 0.09) & (u < 0.10), -v, v)
        raw[t] = v.astype(np.int32)
    return raw, luma, truth


def static_part(truth: np.ndarray) -> np.ndarray:
    """(H,W) bool: the pixels of a clip whose truth never changes (the moving square never covers them)."""
    return np.all(truth == truth[0], axis=0)


def flicker(maps: np.ndarray) -> float:
    """mean |m_t - m_{t-1}| over the pixels that are > 0 in both frames, in raw units (nan without such a pixel)."""
    m = np.asarray(maps).astype(np.int64)
    both = (m[1:] > 0) & (m[:-1] > 0)
    return float(np.abs(m[1:] - m[:-1])[both].mean()) if both.any() else float("nan")
