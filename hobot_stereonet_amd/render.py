"""Twin of the reference's render node:
``stereonet_render_tools/hobot_stereonet_render/publisher_member_function.py:45-163`` —
``MinimalPublisher.listener_callback`` takes the ``/stereonet_node_output`` payload (int32 tensor ‖ JPEG of
the left eye), turns it into metric depth, colour-maps it and stacks it under the left image for ``/image_jpeg``.

The reference is Python + cv2 + rclpy; cv2 and rclpy are not installed here, so this twin is numpy + PIL and
re-states the three cv2 calls it needs:
  * ``cv2.convertScaleAbs(src, alpha)``  = saturate_cast<uint8>(|src*alpha|), round-half-even, NaN -> 0, inf -> 255
  * ``cv2.applyColorMap(_, COLORMAP_JET)`` = 256-entry LUT r,g,b(x = i/255) = clip(1.5 - |4x - {3,2,1}|, 0, 1)
    (checked against the two table values remembered from OpenCV's colormap.cpp: r[96] = 0.00588235…,
    r[97] = 0.02156862…); PARITY UNPINNED — no cv2 in this image to diff the table or the JPEG bytes against.
  * ``cv2.imdecode`` / ``cv2.imencode('.jpg')`` -> PIL (default cv2 quality 95).
Quirks reproduced on purpose: the payload is viewed as **uint32**; the colour map
goes through a BGR-as-RGB PIL round trip, so its red and blue channels end up swapped in the published image.
"""
from __future__ import annotations

import io
from typing import Tuple

import numpy as np

SCALE = 0.00000260443857769133      # publisher_member_function.py:29
FOCAL = 527.1931762695312           # :30
BASELINE = 119.89382172             # :31


def jet_lut() -> np.ndarray:
    """COLORMAP_JET as a (256, 3) uint8 table in cv2's BGR channel order."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4.0 * x - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * x - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * x - 1.0), 0.0, 1.0)
    return np.rint(np.stack([b, g, r], axis=1) * 255.0).astype(np.uint8)


def convert_scale_abs(src: np.ndarray, alpha: float) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.abs(np.asarray(src, np.float64) * alpha)
        out = np.where(np.isnan(v), 0.0, np.minimum(np.rint(v), 255.0))
    return out.astype(np.uint8)


def split_payload(data: bytes, w: int, h: int) -> Tuple[np.ndarray, bytes]:
    """:57-66 — first w*h*4 bytes = model output viewed as uint32, rest = JPEG of the left eye."""
    n = w * h * 4
    if len(data) < n:
        raise ValueError("payload shorter than the model output tensor")
    raw = np.frombuffer(data[:n], dtype=np.uint32).reshape(h, w)
    return raw, bytes(data[n:])


def disparity_and_depth(raw_u32: np.ndarray, dmax_factor: float = 16 * 12) -> Tuple[np.ndarray, np.ndarray]:
    """:72-81 — image_pre = raw * scale * 16 * 12 (px); Z = f*B/image_pre/1000 (m); 0 disparity -> inf."""
    disp = raw_u32.astype(np.float64) * SCALE * dmax_factor
    with np.errstate(divide="ignore"):
        depth = FOCAL * BASELINE / disp / 1000.0
    return disp, depth


def colorize_depth(depth: np.ndarray, alpha: float = 9.0) -> np.ndarray:
    """:82 — applyColorMap(convertScaleAbs(Z, alpha=9), COLORMAP_JET) -> (h, w, 3) uint8 in BGR order."""
    return jet_lut()[convert_scale_abs(depth, alpha)]


def render(data: bytes, w: int, h: int):
    """-> (disp float64 (h,w), depth float64 (h,w), joint uint8 (2h, w, 3) RGB as finally published)."""
    from PIL import Image
    raw, jpeg = split_payload(data, w, h)
    disp, depth = disparity_and_depth(raw)
    color_bgr = colorize_depth(depth)
    left_rgb = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))     # :94-101: imdecode (BGR) + r/b swap = RGB
    # :108,121-137: the BGR colour map is handed to PIL as if it were RGB, pasted under the (true RGB) left image
    # and the whole canvas is channel-reversed for cv2.imencode -> in true colours the colour map's R and B swap
    joint = np.concatenate([left_rgb, color_bgr], axis=0)
    return disp, depth, joint


def encode_jpeg(joint_rgb: np.ndarray, quality: int = 95) -> bytes:
    """:159 — cv2.imencode('.jpg') of the stacked image (what goes out on /image_jpeg)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(joint_rgb, "RGB").save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


# ---- the GPU stage "render" (sn_render / sn_render_jpeg, include/stereonet_hip.h): the same picture made from the map and the
# left eye as they lie in device memory.  Everything below is the numpy twin of that contract: no tolerance, the same bytes.
STACK, DEPTH = 0, 1                 # SN_RENDER_STACK / SN_RENDER_DEPTH
RGB8, NV12 = 0, 1                   # SN_RENDER_RGB8 / SN_RENDER_NV12
CMAP_JET, CMAP_GREY = 0, 1          # SN_CMAP_JET / SN_CMAP_GREY
ALPHA = 9.0                         # publisher_member_function.py:82


class RenderParams:
    """sn_render_params: a zero scale / focal_px / baseline_mm / alpha is the reference's value; all zero is the reference's
    render node."""

    def __init__(self, scale: float = 0.0, focal_px: float = 0.0, baseline_mm: float = 0.0, alpha: float = 0.0,
                 layout: int = STACK, colormap: int = CMAP_JET, true_colours: int = 0, invalid_black: int = 0):
        self.scale, self.focal_px, self.baseline_mm, self.alpha = float(scale), float(focal_px), float(baseline_mm), float(alpha)
        self.layout, self.colormap, self.true_colours, self.invalid_black = int(layout), int(colormap), int(true_colours), int(invalid_black)

    def resolved(self) -> Tuple[float, float, float, float]:
        return (self.scale or SCALE, self.focal_px or FOCAL, self.baseline_mm or BASELINE, self.alpha or ALPHA)


def render_tables(params: RenderParams = None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (rgb, ycc), both uint8 (257, 3).  rgb[i] = the canvas bytes (in its R, G, B positions) of colour index i, entry 256
    black; ycc[i] = their JFIF BT.601 YCbCr in libjpeg's fixed point."""
    p = params or RenderParams()
    if p.colormap == CMAP_JET:
        t = jet_lut()
    elif p.colormap == CMAP_GREY:
        t = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    else:
        raise ValueError("render: unknown colour map")
    if p.true_colours:
        t = t[:, ::-1]                 # the map's (B, G, R) -> (R, G, B); otherwise B, G, R are stored as if they were R, G, B
    rgb = np.concatenate([t, np.zeros((1, 3), np.uint8)], axis=0)
    r, g, b = (rgb[:, i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return np.ascontiguousarray(rgb), np.stack([y, cb, cr], axis=1).astype(np.uint8)


def _u32(raw) -> np.ndarray:
    a = np.asarray(raw)
    if a.dtype == np.int32:
        return a.view(np.uint32)
    return a.astype(np.uint32)


def colour_index(raw, params: RenderParams = None) -> np.ndarray:
    """The contract's colour index of map words (viewed as uint32), 0..255, in IEEE double, left to right."""
    scale, focal, baseline, alpha = (params or RenderParams()).resolved()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = _u32(raw).astype(np.float64) * scale * 16.0 * 12.0
        z = focal * baseline / d / 1000.0
        a = np.abs(z * alpha)
        idx = np.where(np.isnan(a), 0.0, np.minimum(np.rint(a), 255.0))
    return idx.astype(np.int64)


def boundary_raws(params: RenderParams = None) -> np.ndarray:
    """uint32: for every i in 0..254 the largest raw whose index exceeds i and that raw plus one (the index never increases as
    raw grows, and raw == 0 gives 255), found by bisection on colour_index; then the specials 0, 1, 2, 0x7fffffff, 0x80000000,
    0xffffffff.  These are the values where a wrong rounding, a float instead of a double or a signed view shows."""
    i = np.arange(255, dtype=np.int64)
    lo = np.zeros(255, np.int64)                 # the index of raw == 0 is 255 > i
    hi = np.full(255, 1 << 32, np.int64)         # beyond the last word: never evaluated
    while np.any(hi - lo > 1):
        mid = (lo + hi) >> 1
        above = colour_index(mid.astype(np.uint32), params) > i
        lo = np.where(above, mid, lo)
        hi = np.where(above, hi, mid)
    pairs = np.stack([lo, np.minimum(lo + 1, 0xffffffff)], axis=1).reshape(-1)
    return np.concatenate([pairs, [0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff]]).astype(np.uint32)


def left_frame_bytes(left_pitch: int, h: int) -> int:
    """Bytes between the left eyes of consecutive frames: h luma rows and ceil(h / 2) chroma rows of left_pitch bytes."""
    return left_pitch * (h + (h + 1) // 2)


def nv12_to_rgb8(nv12, w: int, h: int, pitch: int, n: int = 1) -> np.ndarray:
    """n NV12 frames (frame k at k * left_frame_bytes(pitch, h)) -> uint8 (n, h, w, 3) by the integer BT.601 conversion that
    sn_pointcloud_from_raw documents (true NV12 chroma siting)."""
    from .pointcloud import nv12_to_rgb
    f = np.ascontiguousarray(nv12, np.uint8).reshape(-1)
    base = (np.arange(n) * left_frame_bytes(pitch, h))[:, None, None]
    u, v = np.arange(w)[None, None, :], np.arange(h)[None, :, None]
    uvo = base + pitch * h + (v >> 1) * pitch + (u & ~1)
    c = nv12_to_rgb(f[base + v * pitch + u], f[uvo], f[uvo + 1])
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)


def canvas(raw, left_nv12=None, left_pitch: int = 0, params: RenderParams = None, fmt: int = RGB8) -> np.ndarray:
    """sn_render's canvases at their minimal pitch.  raw int32 / uint32 (H, W) or (n, H, W); left_nv12: n frames at luma pitch
    left_pitch (0: W), frame k at k * left_frame_bytes(left_pitch, H) (the last one may end with its last chroma row); not read
    with layout DEPTH.  -> uint8 (n, Hc, W, 3) for RGB8, (n, Hc * 3 / 2, W) for NV12 (Hc luma rows, then the chroma rows)."""
    p = params or RenderParams()
    r = _u32(raw)
    if r.ndim == 2:
        r = r[None]
    n, h, w = r.shape
    if p.layout not in (STACK, DEPTH) or fmt not in (RGB8, NV12):
        raise ValueError("render: unknown layout or format")
    if fmt == NV12 and ((w | h) & 1):
        raise ValueError("render: the NV12 canvas needs an even width and height")
    stack = p.layout == STACK
    pitch = left_pitch or w
    if stack and (left_nv12 is None or pitch < w or (pitch & 1)):
        raise ValueError("render: the stacked canvas needs a left eye at an even pitch >= W")
    rgb, ycc = render_tables(p)
    idx = colour_index(r, p)
    if p.invalid_black:
        idx = np.where(r == 0, 256, idx)
    if fmt == RGB8:
        colour = rgb[idx]
        return np.concatenate([nv12_to_rgb8(left_nv12, w, h, pitch, n), colour], axis=1) if stack else colour
    t = ycc[idx].astype(np.int64)
    y = t[..., 0].astype(np.uint8)
    c = (t[:, 0::2, 0::2, 1:] + t[:, 0::2, 1::2, 1:] + t[:, 1::2, 0::2, 1:] + t[:, 1::2, 1::2, 1:] + 2) >> 2
    uv = c.astype(np.uint8).reshape(n, h // 2, w)
    if not stack:
        return np.concatenate([y, uv], axis=1)
    f = np.ascontiguousarray(left_nv12, np.uint8).reshape(-1)
    base = (np.arange(n) * left_frame_bytes(pitch, h))[:, None, None]
    rows = f[base + np.arange(h + h // 2)[None, :, None] * pitch + np.arange(w)[None, None, :]]
    return np.concatenate([rows[:, :h], y, rows[:, h:], uv], axis=1)


def canvas_jpeg(raw, left_nv12=None, left_pitch: int = 0, params: RenderParams = None, quality: int = 95,
                rows_per_slice: int = 1):
    """sn_render_jpeg: jpeg.encode_nv12 of every NV12 canvas -> list of n bytes objects."""
    from . import jpeg
    c = canvas(raw, left_nv12, left_pitch, params, NV12)
    w, hc = c.shape[2], c.shape[1] * 2 // 3
    return [jpeg.encode_nv12(f, w, hc, w, quality, rows_per_slice) for f in c]
