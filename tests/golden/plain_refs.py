"""The independent second implementations the CPU tests judge the numpy twins by, each written from the contract in
include/stereonet_hip.h one pixel (point, frame) at a time: the flood fill and scalar fill of the speckle filter, the per-pixel
loops of the smoother and the temporal filter, the scalar contract of the left-right check, the obstacle grid's scalar loop, and
the host C++ canvas of the render node.  tests/test_dispfilter.py, test_smooth.py, test_temporal.py, test_lrcheck.py,
test_obstacles.py and test_render_canvas.py use them on their own inputs, tests/test_postproc_domain.py on the geometries of
tests/golden/postproc_domain.py.  Nothing here imports a twin's arithmetic."""
import ctypes as C
import functools
import itertools
import math
import os
import subprocess

import numpy as np

from hobot_stereonet_amd import lrcheck, render, spec
from hobot_stereonet_amd.dispfilter import FILLED, SPECKLE
from hobot_stereonet_amd.dispfilter import INVALID_IN as FLT_INVALID_IN
from hobot_stereonet_amd.lrcheck import INCONSISTENT, KEPT, NO_PARTNER, OUT_OF_VIEW
from hobot_stereonet_amd.lrcheck import INVALID_IN as LRC_INVALID_IN
from hobot_stereonet_amd.temporal import BLENDED, HELD, JUMP, MOVED
from hobot_stereonet_amd.temporal import INVALID_IN as TMP_INVALID_IN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
IMAX = 2 ** 31 - 1
INT32_MIN = -(1 << 31)
f32 = np.float32


# ---- sn_filter_raw ---------------------------------------------------------------------------------------------------------------
def flood_speckles(raw, dq, max_px):
    """The contract's stage 1 by flood fill, Python integers throughout -> (M, removed)."""
    H, W = raw.shape
    seen = np.zeros((H, W), bool)
    M = np.where(raw > 0, raw, 0).astype(np.int32)
    removed = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if raw[y, x] <= 0 or seen[y, x]:
                continue
            stack, comp = [(y, x)], []
            seen[y, x] = True
            while stack:
                a, b = stack.pop()
                comp.append((a, b))
                for c, d in ((a + 1, b), (a - 1, b), (a, b + 1), (a, b - 1)):
                    if 0 <= c < H and 0 <= d < W and not seen[c, d] and raw[c, d] > 0 and \
                            abs(int(raw[a, b]) - int(raw[c, d])) <= dq:
                        seen[c, d] = True
                        stack.append((c, d))
            if len(comp) <= max_px:
                for a, b in comp:
                    M[a, b] = 0
                    removed[a, b] = True
    return M, removed


def scalar_fill(M, fill_max):
    """The contract's stage 2, one pixel at a time -> (out, filled)."""
    H, W = M.shape
    out = M.copy()
    filled = np.zeros((H, W), bool)
    for v in range(H):
        for u in range(W):
            if M[v, u] > 0:
                continue
            ul = next((x for x in range(u - 1, -1, -1) if M[v, x] > 0), None)
            ur = next((x for x in range(u + 1, W) if M[v, x] > 0), None)
            if ul is None and ur is None:
                continue
            gap = (W if ur is None else ur) - (-1 if ul is None else ul) - 1
            if gap <= fill_max:
                out[v, u] = M[v, ur] if ul is None else (M[v, ul] if ur is None else min(M[v, ul], M[v, ur]))
                filled[v, u] = True
    return out, filled


def filter_independent(raw, max_px, dq, fill_max):
    M = np.where(raw > 0, raw, 0).astype(np.int32)
    mask = np.where(raw <= 0, FLT_INVALID_IN, 0).astype(np.uint8)
    if max_px:
        M, removed = flood_speckles(raw, dq, max_px)
        mask[removed] = SPECKLE
    if fill_max:
        M, filled = scalar_fill(M, fill_max)
        mask[filled] |= FILLED
    return M, mask


# ---- sn_smooth_raw ---------------------------------------------------------------------------------------------------------------
def smooth_brute(raw, luma, radius, sigma, min_valid):
    """include/stereonet_hip.h, sn_smooth_raw, word for word: collect the participants, sort, scan."""
    H, W = raw.shape
    s = sigma
    T = [1] * 256 if s == 0 else [(256 * s * s) // (s * s + j * j) for j in range(256)]
    out = np.zeros((H, W), np.int32)
    mask = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            part, measured = [], 0
            for y in range(max(0, v - radius), min(H, v + radius + 1)):
                for x in range(max(0, u - radius), min(W, u + radius + 1)):
                    if raw[y, x] > 0:
                        measured += 1
                        wq = T[abs(int(luma[y, x]) - int(luma[v, u]))] if s else 1
                        if wq > 0:
                            part.append((int(raw[y, x]), wq))
            wt = sum(wq for _, wq in part)
            m = None
            for val in sorted({val for val, _ in part}):
                if 2 * sum(wq for v2, wq in part if v2 <= val) >= wt:
                    m = val
                    break
            if raw[v, u] > 0:
                res = m
            else:
                res = m if (min_valid > 0 and measured >= min_valid and wt > 0) else 0
            out[v, u] = res
            mask[v, u] = (1 if raw[v, u] <= 0 else 0) | (128 if res != max(int(raw[v, u]), 0) else 0)
    return out, mask


# ---- sn_temporal_push ------------------------------------------------------------------------------------------------------------
def temporal_loop(raw, luma, alpha, q, persist, luma_delta):
    """The contract, one pixel and one frame at a time, in Python integers (nothing can overflow)."""
    T, H, W = raw.shape
    out, mask = np.zeros(raw.shape, np.int64), np.zeros(raw.shape, np.uint8)
    for v, u in itertools.product(range(H), range(W)):
        P, Hs, Yp = 0, 0, None
        for t in range(T):
            r, y = max(int(raw[t, v, u]), 0), int(luma[t, v, u])
            moved = luma_delta > 0 and Yp is not None and abs(y - Yp) > luma_delta
            bits = 0
            if r > 0:
                if P > 0 and not moved and abs(r - P) <= q:
                    o = (alpha * r + (256 - alpha) * P + 128) >> 8
                    assert o >= 1
                    bits = BLENDED if o != r else 0
                else:
                    o = r
                    if P > 0:
                        bits = MOVED if moved else JUMP
                P = o
            else:
                bits = TMP_INVALID_IN
                if persist > 0 and P > 0 and not moved and bin(Hs).count("1") >= persist:
                    o = P
                    bits |= HELD
                else:
                    o = 0
                    if P > 0 and moved:
                        bits |= MOVED
                        P = 0
            Hs = ((Hs << 1) | (r > 0)) & 255
            if Hs == 0:
                P = 0
            Yp = y
            out[t, v, u], mask[t, v, u] = o, bits
    assert out.min() >= 0 and out.max() <= IMAX
    return out.astype(np.int32), mask


# ---- sn_lr_check -----------------------------------------------------------------------------------------------------------------
def lrcheck_scalar(L, R, tau_px, tau_rel, mirrored):
    """The contract, one pixel at a time, every operation a float32 scalar operation."""
    S = lrcheck.wire_scale()
    L = np.asarray(L, np.int32)
    R = np.asarray(R, np.int32)
    H, W = L.shape
    mask = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            def Rx(x):
                return int(R[v, W - 1 - x] if mirrored else R[v, x])
            rl = int(L[v, u])
            if rl <= 0:
                mask[v, u] = LRC_INVALID_IN
                continue
            d = f32(rl) * S
            xr = f32(u) - d
            if xr < 0:
                mask[v, u] = OUT_OF_VIEW
                continue
            x0 = int(np.floor(xr))
            t = xr - f32(x0)
            x1 = min(x0 + 1, W - 1)
            r0, r1 = Rx(x0), Rx(x1)
            d0, d1 = f32(r0) * S, f32(r1) * S
            if r0 <= 0 and r1 <= 0:
                mask[v, u] = NO_PARTNER
                continue
            if r0 <= 0:
                dr = d1
            elif r1 <= 0:
                dr = d0
            else:
                dr = d0 + t * (d1 - d0)
            if not (abs(d - dr) <= f32(tau_px) + f32(tau_rel) * d):
                mask[v, u] = INCONSISTENT
    return np.where(mask == KEPT, L, 0).astype(np.int32), mask, np.uint32((mask == KEPT).sum())


# ---- sn_obstacles_from_raw -------------------------------------------------------------------------------------------------------
def obstacles_scalar_loop(raw, cam, p, edges):
    """sn_obstacles_from_raw's contract one point at a time, np.float32 scalars, every operation rounded on its own."""
    n, H, W = raw.shape
    s = cam.step
    Ho, Wo = -(-H // s), -(-W // s)
    m = [f32(v) for v in p.base_from_cam]
    if not any(float(v) != 0.0 for v in m):
        m = [f32(v) for v in (0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0)]
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
    fB = fx * f32(cam.baseline_mm)
    zmin, zmax = f32(cam.z_min_m), f32(cam.z_max_m)
    gw, gh = p.gw, p.gh
    hits = np.zeros((n, gh, gw, 2), np.uint32)
    height = np.full((n, gh, gw), INT32_MIN, np.int64)
    ranges = np.full((n, p.beams), np.inf, f32)
    for k in range(n):
        for i in range(Ho):
            for j in range(Wo):
                u, v = j * s, i * s
                r = int(raw[k, v, u])
                if r <= 0:
                    continue
                dis = f32(r) * f32(spec.OUT_SCALE)
                Z = f32(np.float64(fB) / (np.float64(dis) * 16.0 * 12.0) / 1000.0)
                if not (zmin <= Z and (zmax <= 0 or Z <= zmax)):
                    continue
                X = f32(f32(f32(u) - cx) * Z) / fx
                Y = f32(f32(f32(v) - cy) * Z) / fy
                xb, yb, zb = (f32(f32(f32(m[4 * q] * X) + f32(m[4 * q + 1] * Y)) + f32(m[4 * q + 2] * Z)) + m[4 * q + 3] for q in range(3))
                ground = f32(p.z_floor_m) <= zb <= f32(p.z_lo_m)
                obstacle = f32(p.z_lo_m) < zb <= f32(p.z_hi_m)
                if not (ground or obstacle):
                    continue
                if gw:
                    qx = f32(math.floor(f32(xb - f32(p.x_min_m)) / f32(p.cell_m)))
                    qy = f32(math.floor(f32(yb - f32(p.y_min_m)) / f32(p.cell_m)))
                    if 0 <= qx < f32(gw) and 0 <= qy < f32(gh):
                        hits[k, int(qy), int(qx), 0 if obstacle else 1] += 1
                        if obstacle:
                            height[k, int(qy), int(qx)] = max(height[k, int(qy), int(qx)], math.floor(f32(zb * f32(1000.0))))
                if p.beams and obstacle and xb > 0:
                    t = yb / xb
                    if edges[0] <= t < edges[p.beams]:
                        rr = f32(np.sqrt(f32(f32(xb * xb) + f32(yb * yb))))
                        if f32(p.range_min_m) <= rr <= f32(p.range_max_m):
                            beam = sum(1 for e in edges if e <= t) - 1
                            ranges[k, beam] = min(ranges[k, beam], rr)
    occ = np.full((n, gh, gw), -1, np.int8)
    occ[hits[..., 1] >= p.min_ground_hits] = 0
    occ[hits[..., 0] >= p.min_obstacle_hits] = 100
    stats = np.stack([hits[..., 0].sum(axis=(1, 2)), hits[..., 1].sum(axis=(1, 2)), (occ == 100).sum(axis=(1, 2)), (occ == 0).sum(axis=(1, 2))],
                     axis=1).astype(np.uint32) if gw else np.zeros((n, 4), np.uint32)
    return occ, hits, height.astype(np.int32), ranges, stats


# ---- sn_render: the host C++ canvas of the compat library --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hostlib():
    san = os.environ.get("SN_SANITIZE") == "1"       # scripts/run_sanitized.sh: the ASan + UBSan build of the mirror
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"] + (["asan"] if san else []))
    import torch  # noqa: F401  (before anything that links HIP: one HIP runtime per process, see api.load_library)
    lib = C.CDLL(os.path.join(COMPAT, "build", "asan" if san else "", "libhobot_stereonet_node.so"))
    vp, ci = C.c_void_p, C.c_int
    lib.snhost_render.argtypes = [vp, C.c_long, ci, ci, vp, vp, vp, vp, vp]
    lib.snhost_render_tables.argtypes = [vp, vp, vp, vp]
    lib.snhost_render_canvas.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, ci, vp, ci, C.c_long]
    lib.snhost_jpeg_nv12_sliced.restype = C.c_long
    lib.snhost_jpeg_nv12_sliced.argtypes = [vp, ci, ci, ci, ci, ci, vp, C.c_long]
    return lib


def render_params_arrays(p):
    return (np.array([p.scale, p.focal_px, p.baseline_mm, p.alpha], np.float64),
            np.array([p.layout, p.colormap, p.true_colours, p.invalid_black], np.int32))


def host_canvas(n, raw, left, pitch, w, h, p, fmt, pad):
    lib = hostlib()
    hc = h * (2 if p.layout == render.STACK else 1)
    rows = hc + hc // 2 if fmt == render.NV12 else hc
    row_bytes = w if fmt == render.NV12 else 3 * w
    out_pitch = row_bytes + pad
    out = np.full((n, rows, out_pitch), 0x5a, np.uint8)
    dp, ip = render_params_arrays(p)
    rc = lib.snhost_render_canvas(n, raw.ctypes.data, left.ctypes.data if left is not None else None, pitch, w, h, dp.ctypes.data,
                                  ip.ctypes.data, fmt, out.ctypes.data, out_pitch, rows * out_pitch)
    assert rc == 0
    assert np.all(out[:, :, row_bytes:] == 0x5a), "the pitch padding is not written"
    body = out[:, :, :row_bytes]
    return body.reshape(n, hc, w, 3) if fmt == render.RGB8 else body
