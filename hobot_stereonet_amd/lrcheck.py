"""Left-right consistency check: the numpy twin of sn_lr_check / sn_mirror_pair_i8 (include/stereonet_hip.h), bit for bit.

The network is left-referenced, so the right eye's disparity map comes from the same weights: feed `mirror_pair(in6)` (eyes
swapped, every row reversed) and reverse the rows of the result.  `reference` follows every left pixel to its partner in that
map and rejects it when the two disparities disagree: the occluded strip behind a foreground edge, the columns whose match
falls outside the right image, and pixels without a measurement.  A rejected pixel gets raw = 0, which Parse, depth_from_raw
and the point cloud already read as "no measurement".

All arithmetic is float32 with every operation rounded on its own, which is what numpy does and what the kernel
(csrc/sn_lrcheck.hpp) is written to do.
"""
from __future__ import annotations

import numpy as np

KEPT, INVALID_IN, OUT_OF_VIEW, NO_PARTNER, INCONSISTENT = 0, 1, 2, 4, 8      # SN_LRC_* reasons
IN_TENSOR, IN_SBS_NV12 = 0, 1                                                # SN_LRC_IN_*
REASONS = {KEPT: "kept", INVALID_IN: "invalid_in", OUT_OF_VIEW: "out_of_view", NO_PARTNER: "no_partner",
           INCONSISTENT: "inconsistent"}
OUT_SCALE = 2.60443857769133e-6      # sn_io_info.out_scale


def wire_scale(out_scale: float = OUT_SCALE) -> np.float32:
    """S of the contract: pixels of disparity per unit of the int32 map, (float)((double)out_scale * 192.0)."""
    return np.float32(np.float64(np.float32(out_scale)) * 192.0)


def mirror_pair(in6: np.ndarray) -> np.ndarray:
    """int8 (6,H,W) or (n,6,H,W) -> out[k][c][v][u] = in[k][(c + 3) % 6][v][W - 1 - u]: the pair whose left-referenced
    map is the right eye's, column-reversed.  An involution."""
    x = np.asarray(in6)
    if x.ndim not in (3, 4) or x.shape[-3] != 6:
        raise ValueError(f"mirror_pair: shape {x.shape} is not ([n,] 6, H, W)")
    return np.ascontiguousarray(np.roll(x, 3, axis=-3)[..., ::-1])


def reference(raw_l, raw_r, tau_px: float = 1.0, tau_rel: float = 0.0, mirrored: bool = False,
              out_scale: float = OUT_SCALE):
    """sn_lr_check: int32 (H,W) or (n,H,W) maps -> (out_raw int32, mask uint8, kept uint32 (n,)).  `mirrored`: raw_r is stored
    column-reversed (the map of the mirrored pair as the network wrote it)."""
    if not (np.isfinite(tau_px) and np.isfinite(tau_rel) and tau_px >= 0 and tau_rel >= 0):
        raise ValueError("tau_px and tau_rel must be finite and >= 0")
    L = np.ascontiguousarray(raw_l, np.int32)
    R = np.ascontiguousarray(raw_r, np.int32)
    if L.shape != R.shape or L.ndim not in (2, 3):
        raise ValueError(f"maps of shape {L.shape} and {R.shape}")
    single = L.ndim == 2
    if single:
        L, R = L[None], R[None]
    if mirrored:
        R = R[..., ::-1]
    W = L.shape[-1]
    S = wire_scale(out_scale)
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        d = L.astype(f32) * S
        xr = np.arange(W, dtype=f32)[None, None, :] - d
        invalid = L <= 0
        oov = ~invalid & (xr < 0)
        live = ~invalid & ~oov
        x0 = np.where(live, np.floor(xr), 0).astype(np.int64)      # 0 <= xr <= u on live pixels
        t = xr - x0.astype(f32)
        x1 = np.minimum(x0 + 1, W - 1)
        r0 = np.take_along_axis(R, x0, -1)
        r1 = np.take_along_axis(R, x1, -1)
        d0, d1 = r0.astype(f32) * S, r1.astype(f32) * S
        nopart = live & (r0 <= 0) & (r1 <= 0)
        dr = d0 + t * (d1 - d0)
        dr = np.where(r0 <= 0, d1, np.where(r1 <= 0, d0, dr))
        tol = f32(tau_px) + f32(tau_rel) * d
        ok = np.abs(d - dr) <= tol
    mask = np.full(L.shape, INCONSISTENT, np.uint8)
    mask[live & ~nopart & ok] = KEPT
    mask[nopart] = NO_PARTNER
    mask[oov] = OUT_OF_VIEW
    mask[invalid] = INVALID_IN
    out = np.where(mask == KEPT, L, 0).astype(np.int32)
    kept = (mask == KEPT).reshape(L.shape[0], -1).sum(1).astype(np.uint32)
    if single:
        return out[0], mask[0], kept
    return out, mask, kept
