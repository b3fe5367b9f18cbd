"""The depth view's contract on the CPU (sn_render, include/stereonet_hip.h): the tables, the colour index, and the canvas of
the numpy twin (hobot_stereonet_amd/render.py) against the reference-mode twin (StackJoint), against the host C++ twin
(RenderCanvas) and against the host JPEG encoder; then what the picture is worth beside PIL's own encoder.

No tolerance appears except in the picture-quality test: the contract is the same bytes."""
import io
import itertools
import os

import numpy as np
import pytest

from hobot_stereonet_amd import jpeg, render, synth
from plain_refs import host_canvas as _host_canvas, hostlib as _hostlib, render_params_arrays as _params_arrays

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
QUALITY_FILE = os.path.join(ROOT, "profiles", "render_canvas_quality.txt")
# profiles/render_canvas_quality.txt: the mean absolute error of the colour half after our stream (table chroma averaged per 2x2
# block, the project's AAN encoder) over the same error after PIL's encoder (quality 95, 4:2:0) on the RGB8 canvas, the largest of
# the three frames below; measured first, then fixed here with the 10 % the issue allows on top.
MEASURED_QUALITY_RATIO = 1.0356
QUALITY_MARGIN = 0.10


def _content(n, h, w, seed):
    """maps that hold the boundaries of every colour step, zeros, negative words and random uint32"""
    rng = np.random.default_rng(seed)
    b = render.boundary_raws()
    raw = rng.integers(0, 1 << 32, n * h * w, dtype=np.uint64).astype(np.uint32)
    k = min(b.size, raw.size // 2)
    raw[:k] = np.roll(b, seed)[:k]
    raw[k::7] = 0
    return raw.reshape(n, h, w).view(np.int32)


def _left(n, h, w, pitch, seed):
    rng = np.random.default_rng(100 + seed)
    return rng.integers(0, 256, n * render.left_frame_bytes(pitch, h), dtype=np.uint8)


def _ycc_by_hand(r, g, b):
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16)


def test_tables():
    rgb, ycc = render.render_tables(render.RenderParams())
    assert rgb.shape == (257, 3) and ycc.shape == (257, 3) and rgb.dtype == np.uint8 and ycc.dtype == np.uint8
    assert np.array_equal(rgb[:256], render.jet_lut()) and not rgb[256].any()
    true_rgb, _ = render.render_tables(render.RenderParams(true_colours=1))
    assert np.array_equal(true_rgb[:256], render.jet_lut()[:, ::-1])
    grey, grey_ycc = render.render_tables(render.RenderParams(colormap=render.CMAP_GREY))
    assert np.array_equal(grey[:256], np.repeat(np.arange(256)[:, None], 3, axis=1))
    # hand-computed: black, white, the three primaries (grey's 0 and 255; JET has pure blue at index 32 (B, G, R) = (255, 0, 0),
    # stored as canvas R; pure green does not occur in JET, so the formula is checked on its own)
    assert tuple(ycc[256]) == (0, 128, 128) and tuple(grey_ycc[0]) == (0, 128, 128) and tuple(grey_ycc[255]) == (255, 128, 128)
    assert _ycc_by_hand(255, 0, 0) == (76, 85, 255) and _ycc_by_hand(0, 255, 0) == (150, 44, 21) and _ycc_by_hand(0, 0, 255) == (29, 255, 107)
    jet = render.jet_lut()
    i_red = int(np.flatnonzero((jet == (255, 0, 0)).all(axis=1))[0])       # canvas (R, G, B) = (255, 0, 0) in reference mode
    assert tuple(ycc[i_red]) == (76, 85, 255)
    t_ycc = render.render_tables(render.RenderParams(true_colours=1))[1]
    assert tuple(t_ycc[i_red]) == (29, 255, 107)                            # the same entry in true colours is pure blue
    # JET[96] / JET[97] = (B, G, R) (254, 255, 1) / (250, 255, 5): r[96] = 0.00588..., r[97] = 0.02156... of OpenCV's table,
    # and those bytes standing where R, G, B belong; e.g. Y[96] = (19595 * 254 + 38470 * 255 + 7471 + 32768) >> 16 = 14827219 >> 16
    assert tuple(jet[96]) == (254, 255, 1) and tuple(jet[97]) == (250, 255, 5)
    assert tuple(ycc[96]) == (226, 1, 148) and tuple(ycc[97]) == (225, 4, 146)


def test_ycc_needs_no_clamp_over_all_rgb():
    r = np.arange(256, dtype=np.int64)[:, None, None]
    g = np.arange(256, dtype=np.int64)[None, :, None]
    b = np.arange(256, dtype=np.int64)[None, None, :]
    for plane in _ycc_by_hand(r, g, b):
        assert plane.shape == (256, 256, 256) and int(plane.min()) >= 0 and int(plane.max()) <= 255


def test_colour_index_and_boundaries():
    b = render.boundary_raws()
    assert b.dtype == np.uint32 and b.size == 2 * 255 + 6
    assert [int(v) for v in b[-6:]] == [0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff]
    pairs = b[:510].reshape(255, 2)
    idx = render.colour_index(pairs)
    assert np.array_equal(pairs[:, 1], pairs[:, 0] + 1)
    assert np.array_equal(idx[:, 0], np.arange(255) + 1) and np.array_equal(idx[:, 1], np.arange(255))      # every step is bracketed
    rng = np.random.default_rng(5)
    raws = np.concatenate([b, rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                           rng.integers(0, 1 << 16, 50000, dtype=np.uint64).astype(np.uint32)])
    want = render.convert_scale_abs(render.disparity_and_depth(raws)[1], 9)
    got = render.colour_index(raws)
    assert np.array_equal(got, want) and set(np.unique(got)) == set(range(256))
    assert np.array_equal(render.colour_index(raws.view(np.int32)), want)      # the signed map is viewed as uint32
    assert render.colour_index(np.uint32(0)) == 255
    # the signed view would show here: -1 has the magnitude of raw == 1, whose index is 255
    assert render.colour_index(np.uint32(1)) == 255 and render.colour_index(np.int32(-1)) == 0
    assert render.colour_index(np.uint32(0x80000000)) == 0


def test_reference_mode_equals_stack_joint():
    lib = _hostlib()
    w, h = 34, 18
    raw = _content(1, h, w, 2)[0]
    left = _left(1, h, w, w, 2)
    left_rgb = np.ascontiguousarray(render.nv12_to_rgb8(left, w, h, w)[0])
    payload = np.concatenate([raw.reshape(-1).view(np.uint8), np.frombuffer(b"\xff\xd8", np.uint8)])
    color = np.empty((h, w, 3), np.uint8)
    joint = np.empty((2 * h, w, 3), np.uint8)
    assert lib.snhost_render(payload.ctypes.data, payload.size, w, h, None, None, color.ctypes.data, left_rgb.ctypes.data,
                             joint.ctypes.data) == 4 * w * h
    got = render.canvas(raw, left, w, render.RenderParams(), render.RGB8)[0]
    assert np.array_equal(got, joint) and np.array_equal(got[h:], color)
    assert np.array_equal(render.canvas(raw, None, 0, render.RenderParams(layout=render.DEPTH), render.RGB8)[0], color)


FLAGS = list(itertools.product((render.RGB8, render.NV12), (render.STACK, render.DEPTH), (render.CMAP_JET, render.CMAP_GREY), (0, 1), (0, 1)))


@pytest.mark.parametrize("w,h", [(96, 64), (34, 18), (2, 2)])
def test_twin_equals_host_cpp(w, h):
    n = 2
    raw = _content(n, h, w, w)
    for i, (fmt, layout, cmap, tc, ib) in enumerate(FLAGS):
        p = render.RenderParams(layout=layout, colormap=cmap, true_colours=tc, invalid_black=ib)
        for pitch in (w, 2 * w, w + 6):
            left = _left(n, h, w, pitch, i)
            want = render.canvas(raw, left, pitch, p, fmt)
            got = _host_canvas(n, raw, left, pitch, w, h, p, fmt, pad=(0, 6)[(i + pitch) & 1])
            assert got.shape == want.shape and np.array_equal(got, want), (fmt, layout, cmap, tc, ib, pitch)
    # other constants than the reference's
    p = render.RenderParams(scale=3e-6, focal_px=400.0, baseline_mm=60.0, alpha=20.0)
    left = _left(n, h, w, w, 0)
    assert np.array_equal(_host_canvas(n, raw, left, w, w, h, p, render.RGB8, 0), render.canvas(raw, left, w, p, render.RGB8))


def test_twin_equals_host_cpp_1242x375():
    w, h = 1242, 375
    raw = _content(1, h, w, 9)
    for i, (fmt, layout, cmap, tc, ib) in enumerate(f for f in FLAGS if f[0] == render.RGB8):
        p = render.RenderParams(layout=layout, colormap=cmap, true_colours=tc, invalid_black=ib)
        pitch = (w, 2 * w, w + 6)[i % 3]
        left = _left(1, h, w, pitch, i)
        want = render.canvas(raw, left, pitch, p, fmt)
        assert np.array_equal(_host_canvas(1, raw, left, pitch, w, h, p, fmt, pad=(0, 6)[i & 1]), want), (layout, cmap, tc, ib, pitch)
    with pytest.raises(ValueError):
        render.canvas(raw, _left(1, h, w, w, 0), w, render.RenderParams(), render.NV12)
    dp, ip = _params_arrays(render.RenderParams())
    out = np.zeros(8, np.uint8)
    assert _hostlib().snhost_render_canvas(1, raw.ctypes.data, None, w, w, h, dp.ctypes.data, ip.ctypes.data, render.NV12,
                                           out.ctypes.data, w, 8) == -1


def test_host_tables_equal_twin():
    lib = _hostlib()
    for cmap, tc in itertools.product((render.CMAP_JET, render.CMAP_GREY), (0, 1)):
        p = render.RenderParams(colormap=cmap, true_colours=tc)
        dp, ip = _params_arrays(p)
        rgb, ycc = np.empty((257, 3), np.uint8), np.empty((257, 3), np.uint8)
        assert lib.snhost_render_tables(dp.ctypes.data, ip.ctypes.data, rgb.ctypes.data, ycc.ctypes.data) == 0
        want = render.render_tables(p)
        assert np.array_equal(rgb, want[0]) and np.array_equal(ycc, want[1])
    dp, ip = _params_arrays(render.RenderParams(colormap=2))
    assert lib.snhost_render_tables(dp.ctypes.data, ip.ctypes.data, None, None) == -1


def test_canvas_jpeg_equals_host_encoder_on_the_twins_canvas():
    lib = _hostlib()
    w, h, n = 34, 18, 2
    raw = _content(n, h, w, 4)
    left = _left(n, h, w, 2 * w, 4)
    for layout in (render.STACK, render.DEPTH):
        p = render.RenderParams(layout=layout, invalid_black=layout)
        cv = render.canvas(raw, left, 2 * w, p, render.NV12)
        hc = cv.shape[1] * 2 // 3
        for q, rows in ((95, 1), (50, 0)):
            got = render.canvas_jpeg(raw, left, 2 * w, p, q, rows)
            for k in range(n):
                buf = np.empty(1 << 16, np.uint8)
                frame = np.ascontiguousarray(cv[k])
                m = lib.snhost_jpeg_nv12_sliced(frame.ctypes.data, w, hc, w, q, rows, buf.ctypes.data, buf.size)
                assert m > 0 and got[k] == buf[:m].tobytes(), (layout, q, rows, k)


# ---- picture quality --------------------------------------------------------------------------------------------------------
def _quality_frames():
    """(name, raw (H, W), left NV12 at pitch W): a ramp over all indices, the boundaries tiled, a synthetic scene"""
    w, h, d = 96, 64, 48
    b = render.boundary_raws()
    left = np.ascontiguousarray(synth.sbs_nv12_frame(w, h, d, 3).reshape(h + h // 2, 2 * w)[:, :w]).reshape(-1)
    steps = b[:510:2][::-1]                                            # one raw per index 1..255, growing index
    ramp = np.concatenate([[b[1]], steps])[(np.arange(w) * 256) // w]   # index 0 first
    scene = np.rint(synth.disparity_field(w, h, d).astype(np.float64) / (render.SCALE * 192)).astype(np.uint32)
    return [("ramp", np.repeat(ramp[None, :], h, axis=0).astype(np.uint32), left),
            ("boundaries", np.resize(b, (h, w)).astype(np.uint32), left),
            ("scene", scene, left)]


def _quality_ratio(raw, left, quality=95):
    from PIL import Image
    h, w = raw.shape
    rgb = render.canvas(raw, left, w, render.RenderParams(), render.RGB8)[0]
    ours = np.asarray(Image.open(io.BytesIO(render.canvas_jpeg(raw, left, w, render.RenderParams(), quality, 1)[0])).convert("RGB"))
    assert ours.shape == (2 * h, w, 3)
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=quality, subsampling="4:2:0")
    base = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    err = lambda a: float(np.abs(a[h:].astype(np.int64) - rgb[h:].astype(np.int64)).mean())      # noqa: E731
    return err(ours), err(base)


def test_picture_quality_beside_pils_encoder():
    """The decoded colour half of our stream is as close to the RGB8 canvas as PIL's own encoder (the stand-in for the
    reference's cv2.imencode) gets from that canvas: ours <= baseline * (the measured ratio + 10 %)."""
    worst = 0.0
    for name, raw, left in _quality_frames():
        ours, base = _quality_ratio(raw, left)
        print(f"{name}: mean |error| of the colour half: ours {ours:.4f}, PIL {base:.4f}, ratio {ours / base:.4f}")
        assert base > 0
        worst = max(worst, ours / base)
        assert ours <= base * (MEASURED_QUALITY_RATIO + QUALITY_MARGIN), name
    recorded = [l for l in open(QUALITY_FILE).read().splitlines() if l.startswith("largest ratio")]
    assert recorded and abs(float(recorded[0].split()[-1]) - MEASURED_QUALITY_RATIO) < 5e-5
