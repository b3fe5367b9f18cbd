"""sn_render / sn_render_jpeg on the MI355X: the canvases equal the numpy twin's (hobot_stereonet_amd/render.py) byte for byte
over every format, layout, colour map and flag, at aligned and odd addresses, minimal and padded pitches, with guard bytes
untouched; 1242x375 (W % 4 == 2, an odd height); the JPEG equals the twin's stream and the encoder's on the rendered canvas; a
stream that does not fit; every call form; beside inference; end to end from the engine's own map; argument errors; what
sn_destroy leaves behind; the node's /image_jpeg and the filelist tool.

No tolerance appears: the contract is the same bytes."""
import ctypes as C
import functools
import itertools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from hobot_stereonet_amd import api, jpeg, render, synth, weights

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10                  # above the encoder's batch slice of 8 frames, so sn_render_jpeg's walk is exercised
GUARD = 16
ERR_ARG = -1                    # SN_ERR_ARG (include/stereonet_hip.h)
FLAGS = list(itertools.product((render.RGB8, render.NV12), (render.STACK, render.DEPTH), (render.CMAP_JET, render.CMAP_GREY), (0, 1), (0, 1)))


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _content(n, h, w, seed=0):
    """the boundaries of every colour step tiled over one map, a ramp over another, random uint32 words in the rest, zeros and
    negative words among all of them"""
    rng = np.random.default_rng(seed)
    b = render.boundary_raws()
    raw = rng.integers(0, 1 << 32, (n, h * w), dtype=np.uint64).astype(np.uint32)
    raw[0] = np.resize(b, h * w)
    if n > 1:
        raw[1] = np.linspace(0, 3_000_000, h * w).astype(np.uint32)
    raw[:, 5::11] = 0
    raw[:, 7::13] |= 0x80000000
    raw = raw.reshape(n, h, w).view(np.int32)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def _inputs():
    """shared by the tests and never changed: the maps, and side-by-side frames whose left half is the left eye at pitch 2W"""
    raw = _content(MAX_BATCH, H, W)
    sbs = np.stack([synth.sbs_nv12_frame(W, H, D, 40 + k) for k in range(MAX_BATCH)]).reshape(MAX_BATCH, H + H // 2, 2 * W)
    eyes = np.ascontiguousarray(sbs[:, :, :W])
    sbs.setflags(write=False)
    eyes.setflags(write=False)
    return raw, sbs, eyes


@functools.lru_cache(maxsize=None)
def _twin(fmt, layout, cmap, tc, ib):
    raw, _, eyes = _inputs()
    c = render.canvas(raw, eyes, W, render.RenderParams(layout=layout, colormap=cmap, true_colours=tc, invalid_black=ib), fmt)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _twin_jpeg(quality, rows):
    raw, _, eyes = _inputs()
    return tuple(render.canvas_jpeg(raw, eyes, W, render.RenderParams(), quality, rows))


def _geometry(p, fmt, w=W, h=H):
    hc = h * (2 if p.layout == render.STACK else 1)
    return hc, (hc + hc // 2 if fmt == render.NV12 else hc), (w if fmt == render.NV12 else 3 * w)


def _device_render(torch, e, raw, left, left_pitch, p, fmt, pad=0, offset=0, stream=0, raw_shift=0):
    """device mode: `out` starts GUARD + offset bytes into a buffer of 0x5a, rows of row_bytes + pad; raw starts raw_shift bytes
    into its buffer -> the canvases at their minimal pitch, after checking every byte the call must not write"""
    n, h, w = raw.shape
    hc, rows, row_bytes = _geometry(p, fmt, w, h)
    pitch = row_bytes + pad
    d_raw = torch.zeros(raw.size * 4 + raw_shift + 16, dtype=torch.uint8, device="cuda")
    d_raw[raw_shift:raw_shift + raw.size * 4].copy_(torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1).copy()))
    d_left = torch.from_numpy(np.ascontiguousarray(left).reshape(-1).copy()).cuda() if left is not None else None
    d_out = torch.full((2 * GUARD + offset + n * rows * pitch,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.render_device(n, d_raw.data_ptr() + raw_shift, d_left.data_ptr() if d_left is not None else 0, left_pitch, p, fmt,
                    d_out.data_ptr() + GUARD + offset, pitch, rows * pitch, stream=stream)
    if stream:
        torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert np.all(o[:GUARD + offset] == 0x5a) and np.all(o[GUARD + offset + n * rows * pitch - pad:] == 0x5a), "guard bytes around out"
    body = o[GUARD + offset:GUARD + offset + n * rows * pitch].reshape(n, rows, pitch)
    assert np.all(body[:, :, row_bytes:] == 0x5a), "the pitch padding is not written"
    body = body[:, :, :row_bytes]
    return body.reshape(n, hc, w, 3) if fmt == render.RGB8 else body


@pytest.mark.gpu
def test_canvas_bytes_equal_twin(eng):
    import torch
    raw, sbs, eyes = _inputs()
    bad = []
    for fmt, layout, cmap, tc, ib in FLAGS:
        p = render.RenderParams(layout=layout, colormap=cmap, true_colours=tc, invalid_black=ib)
        want = _twin(fmt, layout, cmap, tc, ib)
        # aligned words, 16-byte map loads | the left eye in place in the side-by-side frame, a padded pitch, an odd address and
        # a map base that is 4- but not 16-byte aligned | a padded pitch at an aligned address
        for left, lp, pad, offset, shift in ((eyes, W, 0, 0, 0), (sbs, 2 * W, 6, 1, 4), (sbs, 2 * W, 6, 0, 0), (eyes, W, 0, 3, 8)):
            got = _device_render(torch, eng, raw, left, lp, p, fmt, pad=pad, offset=offset, raw_shift=shift)
            if got.shape != want.shape or not np.array_equal(got, want):
                bad.append((fmt, layout, cmap, tc, ib, lp, pad, offset, shift, int((got != want).sum())))
    print(f"{4 * len(FLAGS)} device calls of n = {MAX_BATCH}, {len(bad)} differ")
    assert not bad, bad
    # other constants than the reference's, n = 1, no left eye at all with the depth layout
    p = render.RenderParams(scale=3e-6, focal_px=400.0, baseline_mm=60.0, alpha=20.0, layout=render.DEPTH)
    assert np.array_equal(_device_render(torch, eng, raw[:1], None, 0, p, render.RGB8), render.canvas(raw[:1], None, 0, p, render.RGB8))


@pytest.mark.gpu
def test_1242x375_rgb8_equals_twin_and_nv12_is_refused(model_factory):
    import torch
    w, h = 1242, 375                                    # W % 4 == 2 and an odd height
    raw = _content(2, h, w, 3)
    pitch = w + 6
    left = np.random.default_rng(8).integers(0, 256, 2 * render.left_frame_bytes(pitch, h), dtype=np.uint8)
    with api.StereoNetHIP(model_factory(w, h, 256), max_batch=2) as e:
        for layout, tc, ib, pad, offset in ((render.STACK, 0, 0, 0, 0), (render.STACK, 1, 1, 6, 1), (render.DEPTH, 0, 1, 0, 2)):
            p = render.RenderParams(layout=layout, true_colours=tc, invalid_black=ib)
            got = _device_render(torch, e, raw, left, pitch, p, render.RGB8, pad=pad, offset=offset)
            assert np.array_equal(got, render.canvas(raw, left, pitch, p, render.RGB8)), (layout, tc, ib, pad, offset)
        assert np.array_equal(e.render(raw, left, pitch), render.canvas(raw, left, pitch))      # host mode
        d_raw = torch.from_numpy(raw.copy()).cuda()
        d_left = torch.from_numpy(left).cuda()
        d_out = torch.full((1 << 20,), 0x5a, dtype=torch.uint8, device="cuda")
        d_sz = torch.full((16,), 0x5a, dtype=torch.uint8, device="cuda")
        prm, jp = api.SnRenderParams(), api.SnJpegParams(95, 1)
        rc = e._lib.sn_render(e._h, 1, d_raw.data_ptr(), d_left.data_ptr(), pitch, C.byref(prm), render.NV12, d_out.data_ptr(), w,
                              w * 3 * h, api.SN_MEM_DEVICE, None)
        assert rc == ERR_ARG and "sn_render" in e._lib.sn_last_error(e._h).decode()
        rc = e._lib.sn_render_jpeg(e._h, 1, d_raw.data_ptr(), d_left.data_ptr(), pitch, C.byref(prm), C.byref(jp), d_out.data_ptr(),
                                   1 << 20, d_sz.data_ptr(), api.SN_MEM_DEVICE, None)
        assert rc == ERR_ARG and "sn_render_jpeg" in e._lib.sn_last_error(e._h).decode()
        torch.cuda.synchronize()
        assert bool((d_out == 0x5a).all()) and bool((d_sz == 0x5a).all())


def _device_jpeg(torch, e, raw, left, left_pitch, p, quality, rows, out_stride, stream=0):
    n = raw.shape[0]
    d_raw = torch.from_numpy(np.ascontiguousarray(raw).copy()).cuda()
    d_left = torch.from_numpy(np.ascontiguousarray(left).reshape(-1).copy()).cuda()
    d_out = torch.full((n * out_stride + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    d_sz = torch.full((n * 4 + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.render_jpeg_device(n, d_raw.data_ptr(), d_left.data_ptr(), left_pitch, p, quality, rows, d_out.data_ptr() + GUARD, out_stride,
                         d_sz.data_ptr() + GUARD, stream=stream)
    if stream:
        torch.cuda.synchronize()
    o, z = d_out.cpu().numpy(), d_sz.cpu().numpy()
    assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + n * out_stride:] == 0x5a), "guard bytes around out"
    assert np.all(z[:GUARD] == 0x5a) and np.all(z[GUARD + n * 4:] == 0x5a), "guard bytes around sizes"
    sizes = z[GUARD:GUARD + n * 4].view(np.uint32)
    body = o[GUARD:GUARD + n * out_stride].reshape(n, out_stride)
    for k in range(n):                                          # nothing behind the stream, nothing at all where it did not fit
        assert np.all(body[k, sizes[k]:] == 0x5a), k
    return [body[k, :sizes[k]].tobytes() if sizes[k] else None for k in range(n)], [int(s) for s in sizes]


@pytest.mark.gpu
def test_render_jpeg_equals_twin_and_the_encoder_on_the_canvas(eng):
    import torch
    raw, sbs, eyes = _inputs()
    p = render.RenderParams()
    cap = api.jpeg_bound(W, 2 * H)
    canvas = eng.render(raw, sbs, 2 * W, p, render.NV12)
    assert np.array_equal(canvas, _twin(render.NV12, render.STACK, render.CMAP_JET, 0, 0))
    for quality, rows in itertools.product((50, 95), (0, 1)):
        want = list(_twin_jpeg(quality, rows))
        assert all(w == jpeg.encode_nv12(_twin(render.NV12, 0, 0, 0, 0)[k], W, 2 * H, W, quality, rows) for k, w in ((0, want[0]), (9, want[9])))
        assert eng.render_jpeg(raw, sbs, 2 * W, p, quality=quality, rows_per_slice=rows) == want, (quality, rows)      # host mode
        dev, sizes = _device_jpeg(torch, eng, raw, sbs, 2 * W, p, quality, rows, cap)
        assert dev == want and sizes == [len(s) for s in want], (quality, rows)
        assert eng.jpeg_encode_nv12(canvas, W, 2 * H, W, n=MAX_BATCH, quality=quality, rows_per_slice=rows) == want
    # the depth layout and the flags reach the stream too
    q = render.RenderParams(layout=render.DEPTH, colormap=render.CMAP_GREY, invalid_black=1)
    assert eng.render_jpeg(raw[:3], None, 0, q, quality=90, rows_per_slice=2) == render.canvas_jpeg(raw[:3], None, 0, q, 90, 2)


@pytest.mark.gpu
def test_render_jpeg_overflow_gives_size_zero_and_writes_nothing(eng):
    import torch
    raw, sbs, _ = _inputs()
    want = list(_twin_jpeg(95, 1))
    longest = max(range(MAX_BATCH), key=lambda k: len(want[k]))
    assert sum(len(w) == len(want[longest]) for w in want) == 1
    stride = len(want[longest]) - 1                     # one byte short of that frame's stream: it alone overflows
    expect = [None if k == longest else want[k] for k in range(MAX_BATCH)]
    dev, sizes = _device_jpeg(torch, eng, raw, sbs, 2 * W, render.RenderParams(), 95, 1, stride)      # asserts the guards and the tails
    assert dev == expect and sizes == [0 if s is None else len(s) for s in expect]
    assert eng.render_jpeg(raw, sbs, 2 * W, None, quality=95, rows_per_slice=1, out_stride=stride) == expect
    dev, _ = _device_jpeg(torch, eng, raw, sbs, 2 * W, render.RenderParams(), 95, 1, stride + 1)       # exactly enough fits
    assert dev == want


@pytest.mark.gpu
def test_every_call_form_gives_the_same_bytes(eng):
    import torch
    raw, sbs, eyes = _inputs()
    side = torch.cuda.Stream()
    for fmt in (render.RGB8, render.NV12):
        want = _twin(fmt, render.STACK, render.CMAP_JET, 0, 0)
        for n in (1, 3, MAX_BATCH):
            assert np.array_equal(eng.render(raw[:n], sbs[:n], 2 * W, None, fmt), want[:n]), (fmt, n)        # host mode
            assert np.array_equal(eng.render(raw[:n], eyes[:n], W, None, fmt), want[:n]), (fmt, n)
            for stream in (0, side.cuda_stream):                                                           # blocking | a caller stream
                got = _device_render(torch, eng, raw[:n], sbs[:n], 2 * W, render.RenderParams(), fmt, stream=stream)
                assert np.array_equal(got, want[:n]), (fmt, n, stream)
        assert np.array_equal(eng.render(raw[0], sbs[0], 2 * W, None, fmt), want[0])                        # a 2-D map
    want = list(_twin_jpeg(95, 1))
    dev, _ = _device_jpeg(torch, eng, raw, sbs, 2 * W, None, 95, 1, api.jpeg_bound(W, 2 * H), stream=side.cuda_stream)
    assert dev == want


@pytest.mark.gpu
def test_render_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread renders (ctypes drops the GIL): the canvases, the streams and the maps
    equal the serial run's."""
    raw, sbs, _ = _inputs()
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    want = _twin(render.RGB8, render.STACK, render.CMAP_JET, 0, 0)[:3]
    want_jpeg = list(_twin_jpeg(95, 1))[:3]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=3) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, rounds = [], []

        def work():
            try:
                for _ in range(12):
                    if not np.array_equal(e.render(raw[:3], sbs[:3], 2 * W), want):
                        errors.append("canvas differs")
                    if e.render_jpeg(raw[:3], sbs[:3], 2 * W) != want_jpeg:
                        errors.append("stream differs")
                    rounds.append(1)
            except Exception as ex:        # noqa: BLE001
                errors.append(repr(ex))

        t = threading.Thread(target=work)
        t.start()
        try:
            for _ in range(5):
                outs = [np.empty((H, W), np.int32) for _ in xs]
                tickets = [e.submit(x, o, None) for x, o in zip(xs, outs)]
                for tk in tickets:
                    e.wait(tk)
                for o, s in zip(outs, serial):
                    assert np.array_equal(o.reshape(s.shape), s)
        finally:
            t.join(60)
        assert not t.is_alive() and not errors and len(rounds) == 12, errors


@pytest.mark.gpu
def test_end_to_end_from_the_engines_own_map(eng):
    sbs = synth.sbs_nv12_frame(W, H, D, 4)
    _, raw = eng.infer_sbs_nv12(sbs)
    raw = raw.reshape(H, W)
    assert len(np.unique(render.colour_index(raw))) > 8             # a picture, not one colour
    for fmt in (render.RGB8, render.NV12):
        assert np.array_equal(eng.render(raw, sbs, 2 * W, None, fmt), render.canvas(raw, sbs, 2 * W, None, fmt)[0])
    assert eng.render_jpeg(raw, sbs, 2 * W) == render.canvas_jpeg(raw, sbs, 2 * W)


@pytest.mark.gpu
def test_argument_errors_write_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    raw, sbs, _ = _inputs()
    HW = H * W
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_left = torch.from_numpy(sbs.reshape(-1).copy()).cuda()
    canvas = 2 * H * 3 * W
    cap = api.jpeg_bound(W, 2 * H)
    d_out = torch.full((MAX_BATCH * max(canvas, cap),), 0x5a, dtype=torch.uint8, device="cuda")
    d_sz = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
    ok = dict(scale=0.0, focal_px=0.0, baseline_mm=0.0, alpha=0.0, layout=0, colormap=0, true_colours=0, invalid_black=0)

    def prm(**kw):
        return api.SnRenderParams(**dict(ok, **kw))

    def call(n=1, r=None, left=None, lp=2 * W, p=prm(), fmt=render.RGB8, out=None, pitch=3 * W, frame=None, mem=api.SN_MEM_DEVICE):
        r = d_raw.data_ptr() if r is None else r
        left = d_left.data_ptr() if left is None else left
        out = d_out.data_ptr() if out is None else out
        rows = 3 * H if fmt == render.NV12 else 2 * H
        frame = rows * pitch if frame is None else frame
        return lib.sn_render(hnd, n, r or None, left or None, lp, C.byref(p) if p is not None else None, fmt, out or None, pitch, frame,
                             mem, None)

    def call_jpeg(n=1, r=None, left=None, lp=2 * W, p=prm(), jp=api.SnJpegParams(95, 1), out=None, stride=cap, sizes=None,
                  mem=api.SN_MEM_DEVICE):
        r = d_raw.data_ptr() if r is None else r
        left = d_left.data_ptr() if left is None else left
        out = d_out.data_ptr() if out is None else out
        sizes = d_sz.data_ptr() if sizes is None else sizes
        return lib.sn_render_jpeg(hnd, n, r or None, left or None, lp, C.byref(p) if p is not None else None,
                                  C.byref(jp) if jp is not None else None, out or None, stride, sizes or None, mem, None)

    assert call() == 0 and call(fmt=render.NV12, pitch=W) == 0 and call_jpeg() == 0      # the baseline calls are fine
    assert call(left=0, p=prm(layout=render.DEPTH), frame=H * 3 * W) == 0                 # the depth layout needs no left eye
    d_out.fill_(0x5a)
    d_sz.fill_(0x5a)
    torch.cuda.synchronize()
    inf, nan = float("inf"), float("nan")
    bad_params = {"unknown layout": prm(layout=2), "unknown colour map": prm(colormap=2), "negative scale": prm(scale=-1e-6),
                  "scale inf": prm(scale=inf), "focal nan": prm(focal_px=nan), "negative focal": prm(focal_px=-1.0),
                  "baseline inf": prm(baseline_mm=inf), "negative baseline": prm(baseline_mm=-2.0), "alpha nan": prm(alpha=nan),
                  "alpha inf": prm(alpha=inf)}
    bad = {"n = 0": dict(n=0), "n > max_batch": dict(n=MAX_BATCH + 1), "null raw": dict(r=0), "null left with the stack": dict(left=0),
           "null params": dict(p=None), "null out": dict(out=0), "bad mem": dict(mem=7), "left_pitch odd": dict(lp=2 * W + 1),
           "left_pitch < W": dict(lp=W - 2), "raw overlaps out": dict(out=d_raw.data_ptr() + 4 * HW - 1),
           "left overlaps out": dict(out=d_left.data_ptr() + 8)}
    bad.update({k: dict(p=v) for k, v in bad_params.items()})
    only_render = {"unknown format": dict(fmt=2), "out_pitch too small": dict(pitch=3 * W - 1), "NV12 out_pitch too small": dict(fmt=render.NV12, pitch=W - 1),
                   "out_frame smaller than a canvas": dict(frame=canvas - 1), "NV12 out_frame too small": dict(fmt=render.NV12, pitch=W, frame=3 * H * W - 1)}
    only_jpeg = {"null jpeg params": dict(jp=None), "null sizes": dict(sizes=0), "out overlaps sizes": dict(sizes=d_out.data_ptr() + 4),
                 "raw overlaps sizes": dict(sizes=d_raw.data_ptr() + 8)}
    for name, kw in {**bad, **only_render}.items():
        rc = call(**kw)
        msg = lib.sn_last_error(hnd).decode()
        assert rc == ERR_ARG and msg.startswith("sn_render: ") and len(msg) > len("sn_render: "), (name, rc, msg)
    for name, kw in {**bad, **only_jpeg}.items():
        rc = call_jpeg(**kw)
        msg = lib.sn_last_error(hnd).decode()
        assert rc == ERR_ARG and msg.startswith("sn_render_jpeg: ") and len(msg) > len("sn_render_jpeg: "), (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((d_out == 0x5a).all()) and bool((d_sz == 0x5a).all())
    with pytest.raises(api.StereoNetError):
        api.render_tables(render.RenderParams(colormap=5))
    for p in (render.RenderParams(), render.RenderParams(colormap=render.CMAP_GREY, true_colours=1)):
        got, want = api.render_tables(p), render.render_tables(p)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_destroy_after_use_leaves_nothing_behind(model_factory):
    """Engines that used the stage in every form are created and closed in turn: the device's free memory does not go down from
    one turn to the next (one turn's scratch and staging is some 30 MB at this size; the slack is a quarter of that)."""
    import torch
    w, h, n = 640, 360, 4
    rng = np.random.default_rng(1)
    raw = rng.integers(1, 1 << 22, (n, h, w), dtype=np.int64).astype(np.int32)
    sbs = np.stack([synth.sbs_nv12_frame(w, h, 96, k) for k in range(n)])
    model = model_factory(w, h, 96)

    def turn():
        with api.StereoNetHIP(model, max_batch=n) as e:
            e.render(raw, sbs, 2 * w, None, render.RGB8)
            e.render(raw, sbs, 2 * w, None, render.NV12)
            e.render_jpeg(raw, sbs, 2 * w, quality=95, rows_per_slice=1)
            d_raw, d_left = torch.from_numpy(raw).cuda(), torch.from_numpy(sbs.reshape(-1)).cuda()
            d_out = torch.empty(n * api.jpeg_bound(w, 2 * h), dtype=torch.uint8, device="cuda")
            d_sz = torch.empty(n, dtype=torch.int32, device="cuda")
            e.render_jpeg_device(n, d_raw.data_ptr(), d_left.data_ptr(), 2 * w, None, 95, 1, d_out.data_ptr(), api.jpeg_bound(w, 2 * h),
                                 d_sz.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        del d_raw, d_left, d_out, d_sz
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    turn()                                  # the runtime's own pools exist after the first
    free = [turn() for _ in range(3)]
    print("free bytes after each turn:", free)
    assert free[2] >= free[0] - (8 << 20), free


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra):
    env = dict(os.environ, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    r = subprocess.run([os.path.join(COMPAT, "build", "render_harness"), model, frames, str(W), str(H), str(nframes), prefix],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    msgs = [open(f"{prefix}.{i}.msg", "rb").read() for i in range(nframes)]
    views = []
    while os.path.exists(f"{prefix}.{len(views)}.render.jpg"):
        i = len(views)
        views.append((open(f"{prefix}.{i}.render.jpg", "rb").read(), open(f"{prefix}.{i}.render.txt").read().split()))
    return msgs, views, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_depth_view(weights_blob, tmp_path):
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 4
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 70 + k) for k in range(nframes)])
    frames.tofile(str(tmp_path / "f.bin"))
    plain, none, _ = _run_harness(tmp_path, "plain", m, str(tmp_path / "f.bin"), nframes, {})
    assert not none                                                      # unset: nothing on /image_jpeg
    for tag, extra, p in (("ref", {}, render.RenderParams()),
                          ("flags", {"STEREONET_RENDER_TRUE": "1", "STEREONET_RENDER_INVALID_BLACK": "1"},
                           render.RenderParams(true_colours=1, invalid_black=1))):
        msgs, views, log = _run_harness(tmp_path, tag, m, str(tmp_path / "f.bin"), nframes, dict(extra, STEREONET_RENDER="95,1"))
        assert msgs == plain, tag                                        # the output messages are byte-identical
        assert len(views) == nframes and "depth view on /image_jpeg" in log
        for k, (data, (frame_id, width, height, step, encoding)) in enumerate(views):
            raw = np.frombuffer(msgs[k][:4 * W * H], np.int32).reshape(H, W)
            assert data == render.canvas_jpeg(raw, frames[k], 2 * W, p, 95, 1)[0], (tag, k)
            assert (int(width), int(height), int(step), encoding) == (W, 2 * H, len(data), "jpeg") and int(frame_id) == 100 + k
    # a value the node refuses leaves it as it is without the variable
    msgs, views, log = _run_harness(tmp_path, "bad", m, str(tmp_path / "f.bin"), nframes, {"STEREONET_RENDER": "95,x"})
    assert msgs == plain and not views and "no depth view" in log


@pytest.mark.gpu
def test_filelist_writes_the_depth_view(model_factory, tmp_path, capsys):
    from PIL import Image
    from hobot_stereonet_amd import filelist, images
    rng = np.random.default_rng(11)
    lists = {}
    for eye in ("left", "right"):
        paths = []
        for i in range(2):
            p = str(tmp_path / f"{eye}{i}.ppm")
            images.write_ppm(p, rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            paths.append(p)
        lists[eye] = str(tmp_path / f"{eye}.list")
        with open(lists[eye], "w") as f:
            f.write("\n".join(paths) + "\n")
    common = ["--model", model_factory(W, H, D), "--left", lists["left"], "--right", lists["right"]]
    out = str(tmp_path / "out")
    assert filelist.main(common + ["--out", out, "--render", "jpeg,90,2", "--render-invalid-black", "--speckle", "40"]) == 0
    total = 0
    p = render.RenderParams(invalid_black=1)
    for i in range(2):
        eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}{i}.ppm"))) for eye in ("left", "right")]
        sbs = images.sbs_from_eyes(eyes[0], eyes[1], W, H)
        raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)      # the final map of the chain
        got = open(os.path.join(out, f"{i}.render.jpg"), "rb").read()
        assert got == render.canvas_jpeg(raw, sbs, 2 * W, p, 90, 2)[0]
        assert Image.open(os.path.join(out, f"{i}.render.jpg")).size == (W, 2 * H)
        total += len(got)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["render_bytes"] == total
    out = str(tmp_path / "out2")
    assert filelist.main(common + ["--out", out, "--render", "ppm", "--render-true-colours"]) == 0
    raw = np.fromfile(os.path.join(out, "0.raw.bin"), np.int32).reshape(H, W)
    eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}0.ppm"))) for eye in ("left", "right")]
    want = render.canvas(raw, images.sbs_from_eyes(eyes[0], eyes[1], W, H), 2 * W, render.RenderParams(true_colours=1))[0]
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "0.render.ppm"))), want)
