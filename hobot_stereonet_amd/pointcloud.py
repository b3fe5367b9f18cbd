"""Point clouds from the int32 disparity map: the camera of ``sn_pointcloud_from_raw`` (include/stereonet_hip.h), a numpy
twin of its arithmetic (bit-exact: every fp32 step rounded as the kernel rounds it), and PLY output.

A point is 16 bytes ``{X, Y, Z, rgb}`` (float32 x 3, then the uint32 ``0x00RRGGBB`` of the PCL packing, 0 without colour).
``points`` arrays are float32 ``(..., 4)``; ``unpack_rgb`` reads the 4th word back as bytes.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np

from . import spec

ORGANISED, COMPACT = 0, 1            # SN_PC_ORGANISED / SN_PC_COMPACT
FOCAL = 527.1931762695312            # the reference's constants (parser.cpp:70-71), as sn_depth_from_raw
BASELINE_MM = 119.89382172
NAN_BITS = 0x7fc00000                # X, Y and Z of an invalid sample of the organised layout


@dataclasses.dataclass
class Camera:
    """sn_camera: pinhole intrinsics of the rectified left eye in pixels of the model's W x H map.  cx / cy left as None
    mean the map's centre (W / 2, H / 2); z_max_m <= 0 means no upper bound."""
    fx: float = FOCAL
    fy: float = FOCAL
    cx: Optional[float] = None
    cy: Optional[float] = None
    baseline_mm: float = BASELINE_MM
    z_min_m: float = 0.0
    z_max_m: float = 0.0
    step: int = 1

    def resolved(self, w: int, h: int) -> "Camera":
        return dataclasses.replace(self, cx=w / 2.0 if self.cx is None else self.cx,
                                   cy=h / 2.0 if self.cy is None else self.cy)

    def out_shape(self, w: int, h: int) -> Tuple[int, int]:
        """(Ho, Wo) = (ceil(H / step), ceil(W / step))"""
        return -(-h // self.step), -(-w // self.step)


def nv12_frame_bytes(pitch: int, h: int) -> int:
    """Bytes of one NV12 frame of luma pitch `pitch`: h luma rows and ceil(h / 2) chroma rows."""
    return pitch * (h + (h + 1) // 2)


def nv12_to_rgb(y, u, v) -> np.ndarray:
    """JFIF full-range BT.601 in integers (arithmetic shifts, clamp to 0..255) -> uint32 0x00RRGGBB."""
    y, uc, vc = (np.asarray(a, np.int64) for a in (y, u, v))
    uc, vc = uc - 128, vc - 128
    r = np.clip(y + ((91881 * vc + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * uc - 46802 * vc + 32768) >> 16), 0, 255)
    b = np.clip(y + ((116130 * uc + 32768) >> 16), 0, 255)
    return ((r << 16) | (g << 8) | b).astype(np.uint32)


def reference(raw: np.ndarray, cam: Camera, layout: int = ORGANISED, nv12: Optional[np.ndarray] = None, pitch: int = 0,
              out_scale: float = spec.OUT_SCALE) -> Tuple[np.ndarray, np.ndarray]:
    """The header's arithmetic on the host.  raw int32 (H, W) or (n, H, W); nv12 uint8, n frames of
    nv12_frame_bytes(pitch, H) bytes (any shape).  -> (points float32, counts uint32 (n,)) with points (n, Ho, Wo, 4) for
    ORGANISED and (n, Ho*Wo, 4) for COMPACT (zeros past each count); leading n dropped when raw is 2-D."""
    r = np.asarray(raw, np.int32)
    single = r.ndim == 2
    if single:
        r = r[None]
    n, h, w = r.shape
    cam = cam.resolved(w, h)
    s = cam.step
    ho, wo = cam.out_shape(w, h)
    rs = r[:, ::s, ::s]
    f32 = np.float32
    dis = rs.astype(f32) * f32(out_scale)
    fb = f32(cam.fx) * f32(cam.baseline_mm)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = (np.float64(fb) / (dis.astype(np.float64) * 16.0 * 12.0) / 1000.0).astype(f32)
        u = (np.arange(wo) * s).astype(f32)[None, None, :]
        v = (np.arange(ho) * s).astype(f32)[None, :, None]
        x = ((u - f32(cam.cx)) * z) / f32(cam.fx)
        y = ((v - f32(cam.cy)) * z) / f32(cam.fy)
    valid = (rs > 0) & (f32(cam.z_min_m) <= z)
    if f32(cam.z_max_m) > 0:
        valid &= z <= f32(cam.z_max_m)
    rgb = np.zeros((n, ho, wo), np.uint32)
    if nv12 is not None:
        fb_ = nv12_frame_bytes(pitch, h)
        fr = np.asarray(nv12, np.uint8).reshape(-1)[:n * fb_].reshape(n, fb_)
        uu = np.arange(wo) * s
        vv = np.arange(ho) * s
        yv = fr[:, (vv[:, None] * pitch + uu[None, :])]
        uvo = pitch * h + (vv[:, None] >> 1) * pitch + (uu[None, :] & ~1)
        rgb = nv12_to_rgb(yv, fr[:, uvo], fr[:, uvo + 1])
    pts = np.stack([x, y, z, rgb.view(f32)], axis=-1)
    counts = valid.reshape(n, -1).sum(axis=1).astype(np.uint32)
    if layout == ORGANISED:
        out = pts.copy()
        out.view(np.uint32)[~valid] = np.array([NAN_BITS, NAN_BITS, NAN_BITS, 0], np.uint32)
    elif layout == COMPACT:
        out = np.zeros((n, ho * wo, 4), f32)
        for k in range(n):
            out[k, :counts[k]] = pts[k][valid[k]]
    else:
        raise ValueError(f"unknown layout {layout}")
    return (out[0], counts[:1]) if single else (out, counts)


def unpack_rgb(points: np.ndarray) -> np.ndarray:
    """(..., 4) float32 points -> (..., 3) uint8 red, green, blue of the 0x00RRGGBB word."""
    c = np.ascontiguousarray(points[..., 3]).view(np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)


def write_ply(path: str, points: np.ndarray, count: Optional[int] = None, colour: bool = True) -> int:
    """Binary little-endian PLY of the first `count` points of a (N, 4) / (Ho, Wo, 4) array (organised input: its finite
    points); vertex = float x y z [+ uchar red green blue].  Returns the number of vertices written."""
    p = np.asarray(points, np.float32).reshape(-1, 4)
    if count is not None:
        p = p[:count]
    p = p[np.isfinite(p[:, 2])]
    dt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colour else [])
    v = np.empty(len(p), dt)
    v["x"], v["y"], v["z"] = p[:, 0], p[:, 1], p[:, 2]
    if colour:
        rgb = unpack_rgb(p)
        v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    props = "".join(f"property {'float' if t == '<f4' else 'uchar'} {name}\n" for name, t in dt)
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\n{props}end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(v.tobytes())
    return len(v)


def read_ply(path: str) -> np.ndarray:
    """The vertices of a PLY written by write_ply, as a numpy structured array."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if head[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = next(int(l.split()[2]) for l in head if l.startswith("element vertex"))
    dt = [(l.split()[2], "<f4" if l.split()[1] == "float" else "u1") for l in head if l.startswith("property")]
    return np.frombuffer(data[end:], dt, count=nv)

