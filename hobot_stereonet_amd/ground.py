"""The ground plane of the int32 disparity map and the mount it implies: the parameters of ``sn_ground_from_raw``
(include/stereonet_hip.h), a numpy twin of its arithmetic (bit-exact: every decision an integer, the two double passages in the
header's order), a plain-loop restatement in Python integers written from the header's text (which also proves the int64
bounds: it cannot overflow), a scene generator with a known answer, the parameter file of the tools and the node, and the
picture ``filelist --ground`` writes.

A plane in space is a plane in (u, v, raw): raw = a*u + b*v + c.  The camera frame is the point cloud's (X right, Y down, Z
forward), the base frame has x forward, y left, z up, a mount is the row-major 3x4 [R|t] of ``obstacles``.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np

from . import paramfile, pointcloud, spec
from .obstacles import LEVEL_MOUNT

MAX_HYPOTHESES, MAX_REFITS = 1024, 4
MAX_RAW = 1 << 24                         # a usable sample: 0 < r <= MAX_RAW
SLOPE_LIM, OFFSET_LIM = 1 << 34, 1 << 41  # |aq|, |bq| and |cq|
FOUND, NO_HYPOTHESIS, FEW_INLIERS, GATED, SINGULAR = 1, 2, 4, 8, 16      # SN_GROUND_*
BITS = {FOUND: "found", NO_HYPOTHESIS: "no_hypothesis", FEW_INLIERS: "few_inliers", GATED: "gated", SINGULAR: "singular"}
LABEL_NONE, LABEL_GROUND, LABEL_ABOVE, LABEL_BELOW, LABEL_NO_PLANE = 0, 1, 2, 3, 4

# sn_ground: one record per map
RECORD = np.dtype([("flags", np.uint32), ("usable", np.uint32), ("inliers", np.uint32), ("winner", np.int32), ("survivors", np.uint32),
                   ("reserved", np.uint32), ("plane_q16", np.int64, 3), ("plane_cam", np.float32, 4), ("base_from_cam", np.float32, 12)])
MOUNT_OFFSET_FLOATS, RECORD_FLOATS = 16, 28      # base_from_cam inside the record, and the record's size, in floats


@dataclasses.dataclass
class GroundParams:
    """sn_ground_params.  base_from_cam: the prior mount (all twelve zero: the level forward mount).  roi all zero: the lower
    half of the image at full width.  log_delta is the node's (not part of the struct): it logs height and tilt when they
    change by more than this many metres or radians."""
    base_from_cam: Tuple[float, ...] = (0.0,) * 12
    roi_x: int = 0
    roi_y: int = 0
    roi_w: int = 0
    roi_h: int = 0
    hypotheses: int = 256
    seed: int = 1
    min_area: int = 64
    min_inliers: int = 100
    refits: int = 2
    tol_px: float = 0.1
    max_tilt_rad: float = 0.5
    height_min_m: float = 0.1
    height_max_m: float = 3.0
    log_delta: float = 0.02

    def matrix(self) -> np.ndarray:
        m = np.asarray(self.base_from_cam, np.float32).reshape(12)
        return np.asarray(LEVEL_MOUNT, np.float32) if not m.any() else m


_FLOATS = ("tol_px", "max_tilt_rad", "height_min_m", "height_max_m", "log_delta")
_INTS = ("roi_x", "roi_y", "roi_w", "roi_h", "hypotheses", "seed", "min_area", "min_inliers", "refits")


def wire_scale(out_scale: float = spec.OUT_SCALE) -> np.float32:
    """S = (float)((double)out_scale * 192.0)"""
    return np.float32(np.float64(np.float32(out_scale)) * 192.0)


def tol_raw(p: GroundParams, out_scale: float = spec.OUT_SCALE) -> int:
    """(int64)floorf(tol_px / S)"""
    return int(np.floor(np.float32(p.tol_px) / wire_scale(out_scale)))


@dataclasses.dataclass(frozen=True)
class Roi:
    """the region's sample grid: samples (j0 + sj, i0 + si) at (u, v) = (j*step, i*step), the centre (u0, v0)"""
    j0: int
    i0: int
    ws: int
    hs: int
    u0: int
    v0: int


def roi(p: GroundParams, w: int, h: int, step: int) -> Roi:
    x, y, rw, rh = p.roi_x, p.roi_y, p.roi_w, p.roi_h
    if not (x or y or rw or rh):
        y, rw, rh = h // 2, w, h - h // 2
    if x < 0 or y < 0 or rw < 1 or rh < 1 or x > w - rw or y > h - rh:
        raise ValueError("the region of interest must lie inside the image")
    j0, i0 = -(-x // step), -(-y // step)
    ws, hs = -(-(x + rw) // step) - j0, -(-(y + rh) // step) - i0
    if ws < 1 or hs < 1 or ws * hs < 3:
        raise ValueError("the region of interest must hold at least three samples")
    return Roi(j0, i0, ws, hs, x + rw // 2, y + rh // 2)


def check(p: GroundParams, out_scale: float = spec.OUT_SCALE) -> Optional[str]:
    """None, or why sn_ground_from_raw refuses these parameters (the region apart: roi() says)."""
    vals = list(np.asarray(p.base_from_cam, np.float64).reshape(-1)) + [p.tol_px, p.max_tilt_rad, p.height_min_m, p.height_max_m]
    if len(p.base_from_cam) != 12 or not np.all(np.isfinite(np.asarray(vals, np.float32))):
        return "every parameter must be finite, base_from_cam twelve numbers"
    if not 1 <= p.hypotheses <= MAX_HYPOTHESES:
        return "hypotheses must be 1..1024"
    if not 0 <= p.refits <= MAX_REFITS:
        return "refits must be 0..4"
    if p.min_area < 0 or p.min_inliers < 0:
        return "min_area and min_inliers must not be negative"
    if np.float32(p.tol_px) < 0 or not np.floor(np.float32(p.tol_px) / wire_scale(out_scale)) <= np.float32(MAX_RAW):
        return "tol_px must not be negative, and tol_raw <= 2^24"
    if np.float32(p.max_tilt_rad) < 0 or np.float32(p.max_tilt_rad) > np.float32(1.5):
        return "max_tilt_rad must lie in [0, 1.5]"
    if not np.float32(p.height_min_m) > 0 or np.float32(p.height_max_m) < np.float32(p.height_min_m):
        return "0 < height_min_m <= height_max_m is required"
    return None


def gate(cam: pointcloud.Camera, p: GroundParams, w: int, h: int, out_scale: float = spec.OUT_SCALE) -> np.ndarray:
    """sn_ground_gate on the host: int64 (6,) = Q16 bounds {a min, a max, b min, b max, c min, c max}.  The library's may differ
    by one where its cos / sin differ by an ulp; tests feed the twin the library's."""
    why = check(p, out_scale)
    if why:
        raise ValueError(why)
    c = cam.resolved(w, h)
    r = roi(p, w, h, c.step)
    f32, f64 = np.float32, np.float64
    m = p.matrix().astype(f64)
    s, bm, fx, fy = f64(wire_scale(out_scale)), f64(f32(c.baseline_mm)) / 1000.0, f64(f32(c.fx)), f64(f32(c.fy))
    cx, cy = f64(f32(c.cx)), f64(f32(c.cy))
    x0, y0, n0 = m[0:3], m[4:7], -m[8:11]
    q = []
    for alpha in (0.0, -f64(f32(p.max_tilt_rad)), f64(f32(p.max_tilt_rad))):
        for beta in (0.0, -f64(f32(p.max_tilt_rad)), f64(f32(p.max_tilt_rad))):
            for hgt in (f64(f32(p.height_min_m)), f64(f32(p.height_max_m))):
                n = math.cos(beta) * (math.cos(alpha) * n0 + math.sin(alpha) * y0) + math.sin(beta) * x0
                g = bm / (hgt * s)
                a, b, cp = g * n[0], g * n[1] * fx / fy, g * n[2] * fx
                cc = (cp + a * (f64(r.u0) - cx)) + b * (f64(r.v0) - cy)
                q.append((a * 65536.0, b * 65536.0, cc * 65536.0))
    q = np.asarray(q, f64)
    out = np.empty(6, np.int64)
    for e in range(3):
        lim = float(SLOPE_LIM if e < 2 else OFFSET_LIM)
        out[2 * e] = int(min(max(math.floor(q[:, e].min()), -lim), lim))
        out[2 * e + 1] = int(min(max(math.ceil(q[:, e].max()), -lim), lim))
    return out


def _mix(seed, i):
    """the header's 32-bit mix, on uint64 arrays masked to 32 bits"""
    m = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed) + np.asarray(i, np.uint64) * np.uint64(0x9E3779B9)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def sample_positions(p: GroundParams, r: Roi, step: int):
    """-> (u, v) int64 (K, 3): the pixels of every hypothesis' three samples"""
    pos = (_mix(p.seed, np.arange(3 * p.hypotheses, dtype=np.uint64)) % np.uint64(r.ws * r.hs)).astype(np.int64).reshape(-1, 3)
    return (r.j0 + pos % r.ws) * step, (r.i0 + pos // r.ws) * step


def _q16(x, lim):
    """(int64)floor(x*65536 + 0.5) where |x*65536| <= lim, else None"""
    s = np.float64(x) * np.float64(65536.0)
    if not (s >= -float(lim) and s <= float(lim)):
        return None
    return int(np.floor(s + np.float64(0.5)))


def _solve(mom):
    """the refit's normal equations in double, the header's order -> (a, b, c) as Q16 integers, or None: singular"""
    n_ = int(mom[0])
    if n_ < 3:
        return None
    with np.errstate(all="ignore"):
        n, su, sv, sr, suu, suv, svv, sur, svr = (np.float64(int(v)) for v in mom)
        mu, mv, mr = su / n, sv / n, sr / n
        cuu, cuv, cvv, cur, cvr = suu - su * mu, suv - su * mv, svv - sv * mv, sur - su * mr, svr - sv * mr
        det = cuu * cvv - cuv * cuv
        if not det > 0:
            return None
        a, b = (cur * cvv - cvr * cuv) / det, (cvr * cuu - cur * cuv) / det
        c = (mr - a * mu) - b * mv
    q = (_q16(a, SLOPE_LIM), _q16(b, SLOPE_LIM), _q16(c, OFFSET_LIM))
    return None if None in q else q


def _geometry(q, r: Roi, cam: pointcloud.Camera, m: np.ndarray, s: np.float32):
    """the header's geometry in double -> (plane_cam float32 (4,), mount float32 (12,)), or None: gated"""
    f64 = np.float64
    with np.errstate(all="ignore"):
        a, b, c = (f64(int(v)) / f64(65536.0) for v in q)
        fx, fy = f64(np.float32(cam.fx)), f64(np.float32(cam.fy))
        cp = (c + a * (f64(np.float32(cam.cx)) - f64(r.u0))) + b * (f64(np.float32(cam.cy)) - f64(r.v0))
        w = (a, (b * fy) / fx, cp / fx)
        ln = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        if not (ln > 0 and ln < np.inf):
            return None
        hgt = (f64(np.float32(cam.baseline_mm)) / f64(1000.0)) / (f64(s) * ln)
        z = [-(w[e] / ln) for e in range(3)]
        p0 = [f64(m[e]) for e in range(3)]
        d = (p0[0] * z[0] + p0[1] * z[1]) + p0[2] * z[2]
        x = [p0[e] - d * z[e] for e in range(3)]
        xl = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        if not xl >= 1e-3:
            return None
        x = [v / xl for v in x]
        y = [z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]]
    mount = np.array(x + [m[3]] + y + [m[7]] + z + [hgt]).astype(np.float32)
    mount[3], mount[7] = m[3], m[7]
    return np.array([-z[0], -z[1], -z[2], hgt]).astype(np.float32), mount


def _finish(rec, k, has, stop, winner, survivors, usable, inliers, q, g, p, r, cam, m, s):
    flags = SINGULAR if stop else 0
    plane, mount = np.array([-m[8], -m[9], -m[10], m[11]], np.float32), m.copy()
    if not has:
        flags |= NO_HYPOTHESIS
    elif inliers < p.min_inliers:
        flags |= FEW_INLIERS
    else:
        geo = _geometry(q, r, cam, m, s) if all(int(g[2 * e]) <= q[e] <= int(g[2 * e + 1]) for e in range(3)) else None
        if geo is None:
            flags |= GATED
        else:
            flags |= FOUND
            plane, mount = geo
    rec[k] = (flags, usable, inliers, winner, survivors, 0, q, plane, mount)
    return bool(flags & FOUND)


def _prepare(raw, cam, p, gate_q16, out_scale):
    why = check(p, out_scale)
    if why:
        raise ValueError(why)
    r3 = np.asarray(raw, np.int32)
    single = r3.ndim == 2
    r3 = r3.reshape((-1,) + r3.shape[-2:])
    n, h, w = r3.shape
    c = cam.resolved(w, h)
    r = roi(p, w, h, c.step)
    g = np.asarray(gate(c, p, w, h, out_scale) if gate_q16 is None else gate_q16, np.int64).reshape(6)
    return r3, single, n, h, w, c, r, g


def reference(raw: np.ndarray, cam: pointcloud.Camera, p: GroundParams, gate_q16: Optional[np.ndarray] = None, labels: bool = True,
              out_scale: float = spec.OUT_SCALE):
    """The header's arithmetic on the host.  raw int32 (H, W) or (n, H, W) -> (records RECORD (n,), labels uint8 (n, H, W) or
    None); leading n dropped when raw is 2-D.  gate_q16: the gate to use (the library's, say) instead of gate()."""
    r3, single, n, h, w, c, r, g = _prepare(raw, cam, p, gate_q16, out_scale)
    step, K, tol, s, m = c.step, p.hypotheses, tol_raw(p, out_scale), wire_scale(out_scale), p.matrix()
    hu, hv = sample_positions(p, r, step)
    us = ((r.j0 + np.arange(r.ws)) * step).astype(np.int64)
    vs = ((r.i0 + np.arange(r.hs)) * step).astype(np.int64)
    U, V = np.meshgrid(us, vs)
    rec = np.zeros(n, RECORD)
    lab = np.zeros((n, h, w), np.uint8) if labels else None
    for k in range(n):
        mp = r3[k].astype(np.int64)
        R = mp[np.ix_(vs, us)]
        ok = (R > 0) & (R <= MAX_RAW)
        usable = int(ok.sum())
        hr = mp[hv, hu]                                                   # (K, 3)
        alive = np.all((hr > 0) & (hr <= MAX_RAW), axis=1)
        du1, dv1, dr1 = hu[:, 1] - hu[:, 0], hv[:, 1] - hv[:, 0], hr[:, 1] - hr[:, 0]
        du2, dv2, dr2 = hu[:, 2] - hu[:, 0], hv[:, 2] - hv[:, 0], hr[:, 2] - hr[:, 0]
        A, B, C = dv1 * dr2 - dr1 * dv2, dr1 * du2 - du1 * dr2, du1 * dv2 - dv1 * du2
        neg = C < 0
        A, B, C = np.where(neg, -A, A), np.where(neg, -B, B), np.where(neg, -C, C)
        A, B, C = (np.where(alive, v, 0) for v in (A, B, C))             # a dead hypothesis' words may be anything
        D = A * hu[:, 0] + B * hv[:, 0] + C * np.where(alive, hr[:, 0], 0)
        alive &= (C >= p.min_area) & (C > 0)
        alive &= (g[0] * C <= -A * 65536) & (-A * 65536 <= g[1] * C) & (g[2] * C <= -B * 65536) & (-B * 65536 <= g[3] * C)
        num = D - A * r.u0 - B * r.v0
        for i in np.flatnonzero(alive):                                   # 70 bits: Python integers
            alive[i] = int(g[4]) * int(C[i]) <= int(num[i]) * 65536 <= int(g[5]) * int(C[i])
        counts = np.zeros(K, np.int64)
        Rf, Uf, Vf = R[ok], U[ok], V[ok]
        for i in np.flatnonzero(alive):
            counts[i] = np.count_nonzero(np.abs(A[i] * Uf + B[i] * Vf + C[i] * Rf - D[i]) <= tol * C[i])
        survivors = int(alive.sum())
        has, stop, winner, q, inliers = survivors > 0, False, -1, (0, 0, 0), 0
        if has:
            winner = int(np.flatnonzero(alive)[np.argmax(counts[alive])])      # argmax: the first of the highest
            cf = np.float64(C[winner])
            q = tuple(_q16(np.float64(v) / cf, lim + 1) for v, lim in ((-A[winner], SLOPE_LIM), (-B[winner], SLOPE_LIM), (num[winner], OFFSET_LIM)))
            dU, dV = Uf - r.u0, Vf - r.v0
            for rnd in range(p.refits + 1):
                inl = np.abs(Rf * 65536 - (q[0] * dU + q[1] * dV + q[2])) <= tol * 65536
                inliers = int(inl.sum())
                if rnd == p.refits or stop:
                    continue
                u_, v_, r_ = dU[inl], dV[inl], Rf[inl]
                mom = [inliers] + [int(x.sum()) for x in (u_, v_, r_, u_ * u_, u_ * v_, v_ * v_, u_ * r_, v_ * r_)]
                nxt = _solve(mom)
                if nxt is None:
                    stop = True
                else:
                    q = nxt
        found = _finish(rec, k, has, stop, winner, survivors, usable, inliers, q, g, p, r, c, m, s)
        if labels:
            uu, vv = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
            e = mp * 65536 - (q[0] * (uu - r.u0) + q[1] * (vv - r.v0) + q[2])
            l_ = np.where(np.abs(e) <= tol * 65536, LABEL_GROUND, np.where(e > 0, LABEL_ABOVE, LABEL_BELOW)) if found else \
                np.full((h, w), LABEL_NO_PLANE)
            lab[k] = np.where((mp > 0) & (mp <= MAX_RAW), l_, LABEL_NONE)
    if single:
        return rec[0], (lab[0] if labels else None)
    return rec, lab


def reference_loops(raw: np.ndarray, cam: pointcloud.Camera, p: GroundParams, gate_q16: Optional[np.ndarray] = None,
                    labels: bool = True, out_scale: float = spec.OUT_SCALE):
    """reference() once more as plain loops over Python integers, written from the header's text: slow, for small maps.  Python
    integers do not overflow, so agreement with reference() on maps at the declared limits proves the int64 bounds."""
    r3, single, n, h, w, c, r, g = _prepare(raw, cam, p, gate_q16, out_scale)
    g = [int(v) for v in g]
    step, K, tol, s, m = c.step, p.hypotheses, tol_raw(p, out_scale), wire_scale(out_scale), p.matrix()
    ns = r.ws * r.hs

    def mix(seed, i):
        x = (seed + i * 0x9E3779B9) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    rec = np.zeros(n, RECORD)
    lab = np.zeros((n, h, w), np.uint8) if labels else None
    for k in range(n):
        mp = r3[k]
        samples = [(j * step, i * step, int(mp[i * step, j * step])) for i in range(r.i0, r.i0 + r.hs) for j in range(r.j0, r.j0 + r.ws)]
        good = [t for t in samples if 0 < t[2] <= MAX_RAW]
        best, winner, survivors, plane = -1, -1, 0, None
        for i in range(K):
            P = [samples[mix(p.seed, 3 * i + j) % ns] for j in range(3)]
            if any(not 0 < t[2] <= MAX_RAW for t in P):
                continue
            d1, d2 = [P[1][e] - P[0][e] for e in range(3)], [P[2][e] - P[0][e] for e in range(3)]
            A, B, C = d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]
            if C < 0:
                A, B, C = -A, -B, -C
            D = A * P[0][0] + B * P[0][1] + C * P[0][2]
            if C < max(p.min_area, 1):
                continue
            num = D - A * r.u0 - B * r.v0
            if not (g[0] * C <= -A * 65536 <= g[1] * C and g[2] * C <= -B * 65536 <= g[3] * C and g[4] * C <= num * 65536 <= g[5] * C):
                continue
            survivors += 1
            cnt = sum(1 for (u, v, rr) in good if abs(A * u + B * v + C * rr - D) <= tol * C)
            if cnt > best:
                best, winner, plane = cnt, i, (A, B, C, num)
        has, stop, q, inliers = plane is not None, False, (0, 0, 0), 0
        if has:
            A, B, C, num = plane
            q = tuple(_q16(np.float64(v) / np.float64(C), lim + 1) for v, lim in ((-A, SLOPE_LIM), (-B, SLOPE_LIM), (num, OFFSET_LIM)))
            for rnd in range(p.refits + 1):
                inl = [(u - r.u0, v - r.v0, rr) for (u, v, rr) in good
                       if abs(rr * 65536 - (q[0] * (u - r.u0) + q[1] * (v - r.v0) + q[2])) <= tol * 65536]
                inliers = len(inl)
                if rnd == p.refits or stop:
                    continue
                mom = [inliers] + [sum(f(*t) for t in inl) for f in (
                    lambda u, v, rr: u, lambda u, v, rr: v, lambda u, v, rr: rr, lambda u, v, rr: u * u, lambda u, v, rr: u * v,
                    lambda u, v, rr: v * v, lambda u, v, rr: u * rr, lambda u, v, rr: v * rr)]
                assert all(abs(x) < 1 << 63 for x in mom)
                nxt = _solve(mom)
                if nxt is None:
                    stop = True
                else:
                    q = nxt
        found = _finish(rec, k, has, stop, winner, survivors, len(good), inliers, q, g, p, r, c, m, s)
        if labels:
            for v in range(h):
                for u in range(w):
                    rr = int(mp[v, u])
                    if not 0 < rr <= MAX_RAW:
                        lab[k, v, u] = LABEL_NONE
                    elif not found:
                        lab[k, v, u] = LABEL_NO_PLANE
                    else:
                        e = rr * 65536 - (q[0] * (u - r.u0) + q[1] * (v - r.v0) + q[2])
                        lab[k, v, u] = LABEL_GROUND if abs(e) <= tol * 65536 else (LABEL_ABOVE if e > 0 else LABEL_BELOW)
    if single:
        return rec[0], (lab[0] if labels else None)
    return rec, lab


def angles(mount) -> Tuple[float, float]:
    """(pitch, roll) in radians of a mount: pitch is the angle by which the camera's forward axis points below the horizon,
    roll the angle by which its right axis does (0, 0 for the level mount)."""
    m = np.asarray(mount, np.float64).reshape(12)
    return float(math.asin(max(-1.0, min(1.0, -m[10])))), float(math.asin(max(-1.0, min(1.0, -m[8]))))


def plane_normal(pitch_rad: float, roll_rad: float) -> np.ndarray:
    """the unit downward normal of a level floor in the frame of a camera whose forward axis dips by pitch and whose right axis
    dips by roll: angles() of the mount that a fit of this floor returns gives the two back"""
    nx, nz = math.sin(roll_rad), math.sin(pitch_rad)
    return np.array([nx, math.sqrt(max(0.0, 1.0 - nx * nx - nz * nz)), nz])


def scene(w: int, h: int, cam: pointcloud.Camera, height_m: float, pitch_rad: float = 0.0, roll_rad: float = 0.0,
          wall_z_m: Optional[float] = None, boxes: int = 0, hole_frac: float = 0.0, outlier_frac: float = 0.0, seed: int = 0,
          out_scale: float = spec.OUT_SCALE):
    """A synthetic map with a known answer -> (raw int32 (h, w), ground bool (h, w): the pixels that show the undisturbed
    floor).  A camera height_m above a level floor, pitched down and rolled; a wall at depth wall_z_m (fronto-parallel to the
    camera) hides what lies behind it; `boxes` rectangles stand nearer than the floor they cover; hole_frac of the pixels hold
    no measurement and outlier_frac a random disparity.  The floor's normal in the camera frame is plane_normal(pitch, roll)."""
    rng = np.random.default_rng(seed)
    c = cam.resolved(w, h)
    s = np.float64(wire_scale(out_scale))
    n = plane_normal(pitch_rad, roll_rad)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = n[0] * (u - c.cx) / c.fx + n[1] * (v - c.cy) / c.fy + n[2]            # n . P / Z
    fb = c.fx * c.baseline_mm / 1000.0
    d = np.where(ray > 0, fb * ray / height_m, 0.0)                               # disparity in px of the floor; 0: the sky
    ground = ray > 0
    if wall_z_m is not None:
        dw = fb / wall_z_m
        ground &= d > dw
        d = np.maximum(d, dw)
    for _ in range(boxes):
        bw, bh = int(rng.integers(w // 12 + 1, w // 5 + 2)), int(rng.integers(h // 10 + 1, h // 4 + 2))
        x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(h // 2, h - bh + 1))
        d[y0:y0 + bh, x0:x0 + bw] = max(d[y0 + bh - 1, x0:x0 + bw].max(), 1e-3) * 1.02      # stands on the floor at its lower edge
        ground[y0:y0 + bh, x0:x0 + bw] = False
    raw = np.rint(d / s).astype(np.int64)
    out = rng.random((h, w)) < outlier_frac
    raw[out] = rng.integers(1, max(2, int(raw.max()) * 2), int(out.sum()))
    hole = rng.random((h, w)) < hole_frac
    raw[hole] = 0
    ground &= ~out & ~hole & (raw > 0)
    return np.clip(raw, 0, (1 << 31) - 1).astype(np.int32), ground


# ---- the parameter file: one `key value...` per line, `#` comments, as the obstacle file -------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS, base_from_cam=paramfile.Key(12))


def save_params(path: str, p: GroundParams) -> None:
    """Floats as repr, so load_params(save_params(p)) == p exactly."""
    paramfile.write(path, "ground plane: base_from_cam = the prior mount, row-major 3x4 [R|t] (all zero: level forward mount), metres, radians",
                    _FILE, [(k, getattr(p, k)) for k in ("base_from_cam",) + _FLOATS + _INTS])


def load_params(path: str) -> GroundParams:
    """A key that is missing keeps GroundParams' default; an unknown or repeated key, or a wrong number of values, is an error."""
    return GroundParams(**paramfile.read(path, _FILE))


# ---- what `filelist --ground` writes ------------------------------------------------------------------------------------------
def labels_image(labels: np.ndarray) -> np.ndarray:
    """labels uint8 (H, W) -> a grey picture: no measurement 0, ground 255, above 96, below 160, no plane 48"""
    lut = np.array([0, 255, 96, 160, 48] + [0] * 251, np.uint8)
    return lut[np.asarray(labels, np.uint8)]


def write_record(path: str, rec) -> None:
    """one `key value...` line per field of the record, the mount's angles in degrees after them"""
    pitch, roll = angles(rec["base_from_cam"])
    with open(path, "w") as f:
        f.write(f"flags {int(rec['flags'])} " + " ".join(name for bit, name in BITS.items() if int(rec["flags"]) & bit) + "\n")
        for k in ("usable", "inliers", "winner", "survivors"):
            f.write(f"{k} {int(rec[k])}\n")
        f.write("plane_q16 " + " ".join(str(int(v)) for v in rec["plane_q16"]) + "\n")
        f.write("plane_cam " + " ".join(repr(float(v)) for v in rec["plane_cam"]) + "\n")
        f.write("base_from_cam " + " ".join(repr(float(v)) for v in rec["base_from_cam"]) + "\n")
        f.write(f"pitch_deg {math.degrees(pitch)!r}\nroll_deg {math.degrees(roll)!r}\n")
