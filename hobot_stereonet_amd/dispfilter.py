"""Speckle removal and hole filling of int32 disparity maps: the numpy twin of sn_filter_raw (include/stereonet_hip.h), bit for
bit.

The left-right check (lrcheck.py) zeroes what the right eye does not confirm.  What it leaves behind is small islands of
surviving pixels (speckles) and the holes it cut.  `reference` removes every connected component of at most `speckle_max_px`
pixels — 4-neighbours belong together when both are > 0 and their raw values differ by at most `diff_units(speckle_diff_px)` —
and then fills every row gap of at most `fill_max_px` pixels with the smaller of its two bounding values (the background,
which is what an occlusion hides).  All per-pixel arithmetic is integer, so the kernels (csrc/sn_dispfilter.hpp) have nothing
to round differently.

The labelling is vectorised: every pixel takes the smallest label among its linked neighbours, the root of its old label is
hooked onto that smaller label (so whole trees merge at once), and pointer jumping flattens the trees; a few sweeps label a
map, a serpentine path included.  The label of a component is its smallest pixel index.
"""
from __future__ import annotations

import numpy as np

from .lrcheck import OUT_SCALE, wire_scale

INVALID_IN, SPECKLE, FILLED = 1, 16, 32      # SN_FLT_* bits; 0 = an untouched measurement
BITS = {INVALID_IN: "invalid_in", SPECKLE: "speckle", FILLED: "filled"}


def diff_units(diff_px: float, out_scale: float = OUT_SCALE) -> int:
    """dq of the contract: floor(speckle_diff_px / S) in float32, as an integer of raw units (2^32 and more count as 2^32)."""
    if not (np.isfinite(diff_px) and diff_px >= 0):
        raise ValueError("speckle_diff_px must be finite and >= 0")
    with np.errstate(over="ignore"):
        q = np.floor(np.float32(diff_px) / wire_scale(out_scale))
    return 2 ** 32 if q >= np.float32(2 ** 32) else int(q)


def links(raw: np.ndarray, dq: int):
    """(H,W) int32 -> (horizontal (H,W-1), vertical (H-1,W)) bool: the link between a pixel and its right / lower neighbour."""
    r = raw.astype(np.int64)
    ok = r > 0
    hl = ok[:, 1:] & ok[:, :-1] & (np.abs(r[:, 1:] - r[:, :-1]) <= dq)
    vl = ok[1:] & ok[:-1] & (np.abs(r[1:] - r[:-1]) <= dq)
    return hl, vl


def label(raw: np.ndarray, dq: int) -> np.ndarray:
    """(H,W) int32 -> (H,W) int64: the smallest pixel index (v*W + u) of every pixel's component; invalid pixels keep their own."""
    H, W = raw.shape
    hl, vl = links(raw, dq)
    L = np.arange(H * W, dtype=np.int64)
    big = np.int64(H * W)
    while True:
        l2 = L.reshape(H, W)
        m = l2.copy()
        np.minimum(m[:, 1:], np.where(hl, l2[:, :-1], big), out=m[:, 1:])
        np.minimum(m[:, :-1], np.where(hl, l2[:, 1:], big), out=m[:, :-1])
        np.minimum(m[1:], np.where(vl, l2[:-1], big), out=m[1:])
        np.minimum(m[:-1], np.where(vl, l2[1:], big), out=m[:-1])
        mf = m.ravel()
        ch = mf < L
        if not ch.any():
            return l2
        np.minimum.at(L, L[ch], mf[ch])          # hook the root of the old label onto the smaller one
        L = np.minimum(L, mf)
        while True:                              # pointer jumping: L[p] <= p always, so this ends at the roots
            j = L[L]
            if np.array_equal(j, L):
                break
            L = j


def remove_speckles(raw: np.ndarray, max_px: int, dq: int):
    """Stage 1 on one (H,W) map -> (M int32 with 0 at every invalid pixel, removed bool)."""
    lab = label(raw, dq)
    size = np.bincount(lab.ravel(), minlength=raw.size)
    removed = (raw > 0) & (size[lab] <= max_px)
    return np.where((raw > 0) & ~removed, raw, 0).astype(np.int32), removed


def fill_rows(M: np.ndarray, fill_max_px: int):
    """Stage 2 on (..., W) maps of stage-1 values -> (filled int32, filled-here bool).  Sources are pixels of M only."""
    W = M.shape[-1]
    idx = np.broadcast_to(np.arange(W, dtype=np.int64), M.shape)
    ok = M > 0
    ul = np.maximum.accumulate(np.where(ok, idx, -1), axis=-1)
    ur = np.minimum.accumulate(np.where(ok, idx, W)[..., ::-1], axis=-1)[..., ::-1]
    vl = np.take_along_axis(M, np.clip(ul, 0, W - 1), -1)
    vr = np.take_along_axis(M, np.clip(ur, 0, W - 1), -1)
    fill = ~ok & ((ul >= 0) | (ur < W)) & (ur - ul - 1 <= fill_max_px)
    val = np.where(ul < 0, vr, np.where(ur >= W, vl, np.minimum(vl, vr)))
    return np.where(fill, val, M).astype(np.int32), fill


def reference(raw, speckle_max_px: int = 0, speckle_diff_px: float = 1.0, fill_max_px: int = 0,
              out_scale: float = OUT_SCALE):
    """sn_filter_raw: int32 (H,W) or (n,H,W) -> (out int32, mask uint8, counts uint32 (n,3) = {valid, removed, filled})."""
    r = np.ascontiguousarray(raw, np.int32)
    if r.ndim not in (2, 3):
        raise ValueError(f"maps of shape {r.shape}")
    single = r.ndim == 2
    if single:
        r = r[None]
    n, H, W = r.shape
    if not (0 <= int(speckle_max_px) <= H * W) or fill_max_px < 0 or (speckle_max_px == 0 and fill_max_px == 0):
        raise ValueError("speckle_max_px must lie in 0..H*W, fill_max_px be >= 0, and one of the two stages be on")
    dq = diff_units(speckle_diff_px, out_scale)
    mask = np.where(r <= 0, INVALID_IN, 0).astype(np.uint8)
    M = np.where(r > 0, r, 0).astype(np.int32)
    if speckle_max_px:
        for k in range(n):
            M[k], removed = remove_speckles(r[k], int(speckle_max_px), dq)
            mask[k][removed] = SPECKLE
    if fill_max_px:
        M, filled = fill_rows(M, int(fill_max_px))
        mask[filled] |= FILLED
    counts = np.stack([(M > 0).reshape(n, -1).sum(1), (mask & SPECKLE != 0).reshape(n, -1).sum(1),
                       (mask & FILLED != 0).reshape(n, -1).sum(1)], 1).astype(np.uint32)
    if single:
        return M[0], mask[0], counts
    return M, mask, counts
