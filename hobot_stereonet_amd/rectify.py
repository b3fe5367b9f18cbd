"""The numpy twin of sn_rectify (include/stereonet_hip.h): stereo rectification of raw NV12 pairs from the camera calibration.

Stage A, `build_map`, is float64 in exactly the header's order of operations (numpy rounds every operation on its own, as the
C++ builder does under `fp contract(off)`), so the maps agree word for word; Stage B, `remap_nv12`, is integer.  Everything the
GPU writes can therefore be compared bit for bit.  `stereo_rectify` makes a calibration from extrinsics (Bouguet's
construction), `load_calib` / `save_calib` read and write the text form the tools share.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np

from . import paramfile

SENTINEL = -2 ** 31
KEYS = ("size", "left.K", "left.D", "left.R", "right.K", "right.D", "right.R", "P", "baseline_mm")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


@dataclasses.dataclass(frozen=True)
class Eye:
    """sn_eye_calib: source intrinsics, plumb-bob distortion k1 k2 p1 p2 k3, rectifying rotation (row-major, source -> rectified)."""
    fx: float
    fy: float
    cx: float
    cy: float
    d: Tuple[float, ...] = (0.0,) * 5
    R: Tuple[float, ...] = IDENTITY

    def __post_init__(self):
        object.__setattr__(self, "d", tuple(float(v) for v in np.ravel(self.d)))
        object.__setattr__(self, "R", tuple(float(v) for v in np.ravel(self.R)))
        for k in ("fx", "fy", "cx", "cy"):
            object.__setattr__(self, k, float(getattr(self, k)))
        if len(self.d) != 5 or len(self.R) != 9:
            raise ValueError("an eye has 5 distortion coefficients and a 3x3 rotation")


@dataclasses.dataclass(frozen=True)
class Calib:
    """sn_stereo_calib: the raw eyes' size, both eyes, the common rectified projection (pixels of the model's W x H), baseline."""
    src_w: int
    src_h: int
    left: Eye
    right: Eye
    pfx: float
    pfy: float
    pcx: float
    pcy: float
    baseline_mm: float

    def __post_init__(self):
        for k in ("pfx", "pfy", "pcx", "pcy", "baseline_mm"):
            object.__setattr__(self, k, float(getattr(self, k)))

    def eye(self, eye: int) -> Eye:
        return self.right if eye else self.left

    def ok(self) -> bool:
        """the checks of sn_rectify_build_map"""
        vals = [self.pfx, self.pfy, self.pcx, self.pcy, self.baseline_mm]
        for e in (self.left, self.right):
            vals += [e.fx, e.fy, e.cx, e.cy, *e.d, *e.R]
        pos = [self.pfx, self.pfy, self.baseline_mm, self.left.fx, self.left.fy, self.right.fx, self.right.fy]
        return (all(2 <= s <= 8192 and s % 2 == 0 for s in (self.src_w, self.src_h)) and bool(np.all(np.isfinite(vals)))
                and all(v > 0 for v in pos))


def identity(w: int, h: int, baseline_mm: float = 119.89382172) -> Calib:
    """A calibration whose map is exactly mx = 256 u, my = 256 v on a w x h source (unit focal lengths and a zero principal
    point, so that no step of Stage A rounds): the rectified frame is the raw frame, byte for byte."""
    e = Eye(1.0, 1.0, 0.0, 0.0)
    return Calib(w, h, e, e, 1.0, 1.0, 0.0, 0.0, baseline_mm)


def _source_point(c: Calib, eye: int, u, v):
    """Stage A up to (us, vs), and Wc, for arrays u, v (float64): the header's operations in the header's order"""
    e = c.eye(eye)
    R = e.R
    k1, k2, p1, p2, k3 = e.d
    with np.errstate(all="ignore"):
        x = (u - c.pcx) / c.pfx
        y = (v - c.pcy) / c.pfy
        X = R[0] * x + R[3] * y + R[6]
        Y = R[1] * x + R[4] * y + R[7]
        Wc = R[2] * x + R[5] * y + R[8]
        a = X / Wc
        b = Y / Wc
        a2 = a * a
        b2 = b * b
        r2 = a2 + b2
        ab2 = 2.0 * (a * b)
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = a * rad + (p1 * ab2 + p2 * (r2 + 2.0 * a2))
        yd = b * rad + (p1 * (r2 + 2.0 * b2) + p2 * ab2)
        us = e.fx * xd + e.cx
        vs = e.fy * yd + e.cy
    return us, vs, Wc


def build_map(calib: Calib, eye: int, w: int, h: int) -> np.ndarray:
    """Stage A: int32 (h, w, 2) = (mx, my) in 1/256 source pixel, (SENTINEL, SENTINEL) where the pixel has no source"""
    if not calib.ok() or eye not in (0, 1) or w < 1 or h < 1:
        raise ValueError("bad calibration, eye or size")
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    us, vs, Wc = _source_point(calib, eye, u, v)
    us, vs, Wc = np.broadcast_to(us, (h, w)), np.broadcast_to(vs, (h, w)), np.broadcast_to(Wc, (h, w))
    with np.errstate(invalid="ignore"):
        ok = (Wc > 0) & (us > -1) & (us < float(calib.src_w)) & (vs > -1) & (vs < float(calib.src_h))
        mx = np.floor(np.where(ok, us, 0.0) * 256.0 + 0.5)
        my = np.floor(np.where(ok, vs, 0.0) * 256.0 + 0.5)
    out = np.full((h, w, 2), SENTINEL, np.int32)
    out[..., 0][ok] = mx[ok].astype(np.int32)
    out[..., 1][ok] = my[ok].astype(np.int32)
    return out


def map_point(calib: Calib, eye: int, u, v):
    """Stage A at real-valued (u, v) without the rounding -> (us, vs) float64 source coordinates (nan behind the camera)"""
    us, vs, Wc = _source_point(calib, eye, np.asarray(u, np.float64), np.asarray(v, np.float64))
    bad = ~(Wc > 0)
    return np.where(bad, np.nan, us), np.where(bad, np.nan, vs)


def is_sentinel(m: np.ndarray) -> np.ndarray:
    return (m[..., 0] == SENTINEL) & (m[..., 1] == SENTINEL)


def remap_plane(plane: np.ndarray, mx: np.ndarray, my: np.ndarray, sentinel: np.ndarray, border: int) -> np.ndarray:
    """Stage B on one plane: plane uint8 (n, ph, pw); mx, my int (h, w) Q8 coordinates on it -> uint8 (n, h, w)"""
    n, ph, pw = plane.shape
    mx, my = mx.astype(np.int64), my.astype(np.int64)
    x0, y0, fx, fy = mx >> 8, my >> 8, mx & 255, my & 255
    acc = np.full((n,) + mx.shape, 32768, np.int64)
    for i, j, wt in ((0, 0, (256 - fx) * (256 - fy)), (1, 0, fx * (256 - fy)), (0, 1, (256 - fx) * fy), (1, 1, fx * fy)):
        x, y = x0 + i, y0 + j
        inside = (x >= 0) & (x < pw) & (y >= 0) & (y < ph)
        p = plane[:, np.clip(y, 0, ph - 1), np.clip(x, 0, pw - 1)].astype(np.int64)
        acc += wt * np.where(inside, p, border)
    out = (acc >> 16).astype(np.uint8)
    out[:, sentinel] = border
    return out


def eye_view(buf: np.ndarray, offset: int, n: int, frame: int, pitch: int, sw: int, sh: int) -> np.ndarray:
    """the (n, sh * 3/2, sw) bytes of one eye in a flat uint8 buffer: pair k's eye starts at offset + k * frame"""
    flat = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    rows = sh + sh // 2
    need = offset + (n - 1) * frame + (rows - 1) * pitch + sw
    if pitch < sw or flat.size < need:
        raise ValueError(f"{n} eyes of {sw}x{sh} at pitch {pitch} take {need} bytes, the buffer has {flat.size}")
    return np.lib.stride_tricks.as_strided(flat[offset:], (n, rows, sw), (frame, pitch, 1), writeable=False)


def remap_nv12(maps, left: np.ndarray, right: np.ndarray, sw: int, sh: int) -> np.ndarray:
    """Stage B: maps = (left map, right map), each int32 (H, W, 2); left, right uint8 (n, sh * 3/2, sw) NV12 eyes ->
    uint8 (n, H * 3/2, 2W) side-by-side NV12 frames"""
    H, W = maps[0].shape[:2]
    n = left.shape[0]
    out = np.empty((n, H + H // 2, 2 * W), np.uint8)
    for eye, (m, src) in enumerate(zip(maps, (left, right))):
        m = np.asarray(m)
        out[:, :H, eye * W:(eye + 1) * W] = remap_plane(src[:, :sh], m[..., 0], m[..., 1], is_sentinel(m), 0)
        mc = m[0::2, 0::2]                                   # chroma sample (cj, ci) takes the luma entry at (2cj, 2ci)
        sent = is_sentinel(mc)
        cx, cy = mc[..., 0].astype(np.int64) >> 1, mc[..., 1].astype(np.int64) >> 1
        for ch in (0, 1):
            out[:, H:, eye * W + ch:(eye + 1) * W:2] = remap_plane(src[:, sh:, ch::2], cx, cy, sent, 128)
    return out


def reference(calib: Calib, w: int, h: int, left: np.ndarray, right: Optional[np.ndarray] = None, pitch: int = 0, n: int = 1,
              frame: int = 0, maps=None) -> np.ndarray:
    """What sn_rectify_nv12 writes to out_sbs_nv12: uint8 (n, h * 3/2, 2w).  left / right: flat uint8 buffers that start at pair
    0's eye (right None: a side-by-side frame, the right eye sw bytes into the left's rows); pitch (0: sw, or 2 sw for a
    side-by-side frame) and frame (0: pitch * sh * 3/2) as the call's src_pitch and src_frame."""
    sw, sh = calib.src_w, calib.src_h
    pitch = pitch or (2 * sw if right is None else sw)
    frame = frame or pitch * (sh + sh // 2)
    if maps is None:
        maps = (build_map(calib, 0, w, h), build_map(calib, 1, w, h))
    le = eye_view(left, 0, n, frame, pitch, sw, sh)
    re = eye_view(left, sw, n, frame, pitch, sw, sh) if right is None else eye_view(right, 0, n, frame, pitch, sw, sh)
    return remap_nv12(maps, le, re, sw, sh)


def tensor_from_sbs(sbs: np.ndarray) -> np.ndarray:
    """sn_preprocess_sbs_nv12_batch in numpy: uint8 (n, H * 3/2, 2W) -> int8 (n, 6, H, W).  As the kernel (and the code it
    mirrors), planes 1 and 2 index the eye's chroma bytes as planar quarter-size U then V."""
    n, rows, w2 = sbs.shape
    H, W = rows * 2 // 3, w2 // 2
    out = np.empty((n, 6, H, W), np.uint8)
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    idx = (i // 2) * (W // 2) + j // 2
    for eye in (0, 1):
        e = sbs[:, :, eye * W:(eye + 1) * W]
        out[:, 3 * eye] = e[:, :H]
        c = np.ascontiguousarray(e[:, H:]).reshape(n, -1)
        out[:, 3 * eye + 1] = c[:, idx]
        out[:, 3 * eye + 2] = c[:, idx + (W * H) // 4]
    return (out ^ np.uint8(0x80)).view(np.int8)


def sbs_to_rgb(sbs: np.ndarray) -> np.ndarray:
    """one side-by-side NV12 frame uint8 (H * 3/2, 2W) -> uint8 (H, 2W, 3) RGB, the point cloud's conversion"""
    from . import pointcloud
    rows, w2 = sbs.shape
    H = rows * 2 // 3
    uv = sbs[H:].reshape(H // 2, w2 // 2, 2)
    u, v = (np.repeat(np.repeat(uv[..., c], 2, 0), 2, 1) for c in (0, 1))
    rgb = pointcloud.nv12_to_rgb(sbs[:H], u, v)
    return np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], -1).astype(np.uint8)


def nonvacuity(m: np.ndarray, sw: int, sh: int) -> dict:
    """What keeps a comparison on the map `m` (one eye, luma plane sw x sh) from passing on nothing: the share of sentinels,
    the number of pixels with a tap partly outside the source, the share of non-sentinel entries with both fractions non-zero"""
    sent = is_sentinel(m)
    mx, my = m[..., 0][~sent].astype(np.int64), m[..., 1][~sent].astype(np.int64)
    x0, y0 = mx >> 8, my >> 8
    outside = (x0 < 0) | (x0 + 1 >= sw) | (y0 < 0) | (y0 + 1 >= sh)
    both = ((mx & 255) != 0) & ((my & 255) != 0)
    return {"sentinels": float(sent.mean()), "partly_outside": int(outside.sum()), "both_fractions": float(both.mean()) if both.size else 0.0}


# ---- calibration files ------------------------------------------------------------------------------------------------------
_FILE = {k: paramfile.Key(n, int if k == "size" else float) for k, n in zip(KEYS, (2, 4, 5, 9, 4, 5, 9, 4, 1))}


def save_calib(path: str, c: Calib) -> None:
    """One `key v v v...` per line, `#` comments; doubles as repr, so load_calib(save_calib(c)) == c exactly."""
    eyes = [(name + k, v) for name, e in (("left", c.left), ("right", c.right)) for k, v in ((".K", (e.fx, e.fy, e.cx, e.cy)), (".D", e.d), (".R", e.R))]
    paramfile.write(path, "stereo calibration: raw eye size, K = fx fy cx cy, D = k1 k2 p1 p2 k3, R row-major, P = pfx pfy pcx pcy", _FILE,
                    [("size", (c.src_w, c.src_h))] + eyes + [("P", (c.pfx, c.pfy, c.pcx, c.pcy)), ("baseline_mm", c.baseline_mm)])


def load_calib(path: str) -> Calib:
    got = paramfile.read(path, _FILE, required=True)
    eyes = [Eye(*got[s + ".K"], got[s + ".D"], got[s + ".R"]) for s in ("left", "right")]
    return Calib(*got["size"], *eyes, *got["P"], got["baseline_mm"])


# ---- a calibration from extrinsics ----------------------------------------------------------------------------------------------
def rodrigues(om) -> np.ndarray:
    """rotation vector -> 3x3 rotation matrix"""
    om = np.asarray(om, np.float64).reshape(3)
    th = float(np.linalg.norm(om))
    if th < 1e-300:
        return np.eye(3)
    k = om / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rotation_vector(R) -> np.ndarray:
    """3x3 rotation matrix (angle below pi) -> rotation vector"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = float(np.linalg.norm(s)), 0.5 * (np.trace(R) - 1.0)
    if sn < 1e-300:
        return np.zeros(3)
    return s * (np.arctan2(sn, cs) / sn)


def stereo_rectify(K1, D1, K2, D2, R, T, src_size, out_size, zoom: float = 1.0) -> Calib:
    """Bouguet's construction for a rig given by extrinsics X2 = R X1 + T (T in mm): the rotation is split in half between the
    eyes, then both are turned so that the baseline lies along +x (the second eye to the right of the first).  K = (fx, fy, cx,
    cy) or a 3x3 matrix.  The rectified projection is the same for both eyes (zero-disparity form: sn_camera has one cx):
    pfx = pfy = 0.5 (fx1 + fx2) W / sw * zoom, centre ((W - 1) / 2, (H - 1) / 2), baseline_mm = |T|."""
    def k4(K):
        K = np.asarray(K, np.float64)
        return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(4))
    def d5(D):
        D = np.zeros(5) if D is None else np.asarray(D, np.float64).reshape(-1)
        if D.size > 5 and np.any(D[5:] != 0):
            raise ValueError("only the plumb-bob model k1 k2 p1 p2 k3 is supported")
        return tuple(np.concatenate([D[:5], np.zeros(max(0, 5 - D.size))]))
    (sw, sh), (W, H) = src_size, out_size
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    r_r = rodrigues(-0.5 * rotation_vector(R))               # R^(-1/2): each eye takes half of the rotation
    t = r_r @ T
    nt = float(np.linalg.norm(t))
    if not t[0] < 0:
        raise ValueError("the second eye must lie to the right of the first (T mostly along -x)")
    uu = np.array([-1.0, 0.0, 0.0])                          # the rectified cam2 = cam1 + (-|T|, 0, 0)
    ww = np.cross(t, uu)
    nw = float(np.linalg.norm(ww))
    if nw > 0:
        ww = ww * (np.arccos(min(1.0, abs(t[0]) / nt)) / nw)
    wR = rodrigues(ww)
    R1, R2 = wR @ r_r.T, wR @ r_r
    k1, k2 = k4(K1), k4(K2)
    f = 0.5 * (k1[0] + k2[0]) * W / sw * zoom
    return Calib(int(sw), int(sh), Eye(*k1, d5(D1), tuple(R1.reshape(9))), Eye(*k2, d5(D2), tuple(R2.reshape(9))),
                 f, f, (W - 1) / 2, (H - 1) / 2, nt)


# ---- test rigs --------------------------------------------------------------------------------------------------------------
def synthetic_rig(sw: int, sh: int, w: int, h: int, seed: int, zoom: float = 0.8, with_extrinsics: bool = False):
    """A random rig for the tests and the benchmark: focal length 0.8 sw with a few per cent of spread, strong barrel distortion
    with tangential terms, rotations of a few degrees between the eyes, T = 120 mm mostly along -x, rectified by stereo_rectify.
    zoom < 1 keeps the borders of the raw eyes in view, so that the maps hold sentinels and taps partly outside the source."""
    rng = np.random.default_rng(seed)
    f = 0.8 * sw
    K = [(f * (1 + 0.02 * rng.standard_normal()), f * (1 + 0.02 * rng.standard_normal()), sw / 2 + 3 * rng.standard_normal(),
          sh / 2 + 3 * rng.standard_normal()) for _ in range(2)]
    D = [(-0.28, 0.09, 0.001, -0.002, -0.01), (-0.25, 0.07, -0.001, 0.001, -0.008)]
    R = rodrigues(np.deg2rad(3.0) * rng.standard_normal(3))
    T = np.array([-120.0, 2.0 * rng.standard_normal(), 3.0 * rng.standard_normal()])
    c = stereo_rectify(K[0], D[0], K[1], D[1], R, T, (sw, sh), (w, h), zoom)
    return (c, K, D, R, T) if with_extrinsics else c


def behind_rig(sw: int, sh: int, w: int, h: int) -> Calib:
    """A wide rectified view turned 60 degrees about y: for the left part of the image Wc <= 0, the source lies behind the camera."""
    Ry = rodrigues((0.0, np.deg2rad(60.0), 0.0))
    e = Eye(0.5 * sw, 0.5 * sw, sw / 2 - 0.25, sh / 2 + 0.125, (-0.05, 0.01, 0.0005, -0.0005, 0.0), tuple(Ry.reshape(9)))
    return Calib(sw, sh, e, dataclasses.replace(e, R=tuple(Ry.T.reshape(9))), w / 5.0, w / 5.0, (w - 1) / 2, (h - 1) / 2, 100.0)
