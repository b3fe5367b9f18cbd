"""sn_rectify on the MI355X: the remap kernel equals the numpy twin (hobot_stereonet_amd/rectify.py) byte for byte — the
side-by-side frame and the int8 tensor — for two model sizes, three sources, side-by-side and separate eyes, unaligned source
addresses, batches, host and device buffers; the device map equals the host builder; every call form gives the same bytes; the
rectified frame composes with inference, the point cloud and the file-list harness; argument errors.  The twin's answers are
computed once per case.

No tolerance appears: Stage A is the same float64 arithmetic on both sides (tests/test_rectify.py), Stage B is integer."""
import ctypes as C
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

from hobot_stereonet_amd import api, rectify, synth

D = {(96, 64): 48, (132, 70): 48, (1280, 720): 192, (1242, 375): 256}
SOURCES = ("identity", "128x80", "160x120")


@functools.lru_cache(maxsize=None)
def _calib(w, h, source):
    if source == "identity":
        return rectify.identity(w, h)
    sw, sh = (int(t) for t in source.split("x"))
    return rectify.synthetic_rig(sw, sh, w, h, sw + w)


@functools.lru_cache(maxsize=None)
def _maps(w, h, source):
    c = _calib(w, h, source)
    maps = tuple(rectify.build_map(c, eye, w, h) for eye in (0, 1))
    for eye, m in enumerate(maps):
        m.setflags(write=False)
        if source != "identity":      # the conditions of tests/test_rectify.py: sentinels, taps partly outside, fractions
            nv = rectify.nonvacuity(m, c.src_w, c.src_h)
            print(f"{w}x{h} from {source} eye {eye}: {nv}")
            assert 0.01 < nv["sentinels"] < 0.50 and nv["partly_outside"] >= 1 and nv["both_fractions"] > 0.90, nv
    return maps


def _sbs_source(sw, sh, n, pitch, seed):
    """n raw side-by-side frames of luma pitch `pitch` (noise beside the eyes too): uint8 (n, sh * 3/2, pitch)"""
    return np.random.default_rng(seed).integers(0, 256, (n, sh + sh // 2, pitch), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(w, h, source, n):
    """-> (raw frames at pitch 2 sw + 16, the twin's rectified frames, the twin's tensors)"""
    c = _calib(w, h, source)
    pitch = 2 * c.src_w + 16
    src = _sbs_source(c.src_w, c.src_h, n, pitch, w + n + c.src_w)
    want = rectify.reference(c, w, h, src, None, pitch, n, maps=_maps(w, h, source))
    ten = rectify.tensor_from_sbs(want)
    for a in (src, want, ten):
        a.setflags(write=False)
    return src, want, ten


def _device_call(torch, r, c, src, n, w, h, separate, stream=0, want_sbs=True, want_tensor=True):
    """device mode with four guard words around every output -> (sbs, tensor).  separate: the eyes as two buffers of pitch sw at
    ODD addresses; else the side-by-side frames as they are, one byte off alignment as well."""
    sw, sh = c.src_w, c.src_h
    rows = sh + sh // 2
    if separate:
        bufs = []
        for eye in (0, 1):
            e = np.ascontiguousarray(src[:, :, eye * sw:(eye + 1) * sw]).reshape(-1)
            d = torch.zeros(e.size + 4, dtype=torch.uint8, device="cuda")
            off = 1 + 2 * eye                                                    # 1 and 3: both odd
            d[off:off + e.size].copy_(torch.from_numpy(e))
            bufs.append((d, d.data_ptr() + off))
        lp, rp, pitch, frame = bufs[0][1], bufs[1][1], sw, sw * rows
    else:
        pitch = src.shape[2]
        d = torch.zeros(src.size + 4, dtype=torch.uint8, device="cuda")
        d[1:1 + src.size].copy_(torch.from_numpy(src.reshape(-1)))
        bufs = [(d, 0)]
        lp, rp, frame = d.data_ptr() + 1, d.data_ptr() + 1 + sw, pitch * rows
    assert (lp | rp) & 1 or not separate
    nb_s, nb_t = n * 3 * w * h, n * 6 * w * h
    d_sbs = torch.full((nb_s + 32,), 0x5a, dtype=torch.uint8, device="cuda")
    d_ten = torch.full((nb_t + 32,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.rectify_device(n, lp, rp, pitch, frame, d_sbs.data_ptr() + 16 if want_sbs else 0, d_ten.data_ptr() + 16 if want_tensor else 0,
                     stream=stream)
    if stream:
        torch.cuda.synchronize()
    s, t = d_sbs.cpu().numpy(), d_ten.cpu().numpy()
    assert np.all(s[:16] == 0x5a) and np.all(s[16 + nb_s:] == 0x5a) and np.all(t[:16] == 0x5a) and np.all(t[16 + nb_t:] == 0x5a)
    if not want_sbs:
        assert np.all(s == 0x5a)
    return s[16:16 + nb_s].reshape(n, h + h // 2, 2 * w), t[16:16 + nb_t].view(np.int8).reshape(n, 6, h, w)


CASES = [(w, h, s) for (w, h) in ((96, 64), (132, 70)) for s in SOURCES]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,source", CASES, ids=[f"{w}x{h}-from-{s}" for w, h, s in CASES])
def test_rectify_kernel_equals_twin_bit_for_bit(model_factory, w, h, source):
    import torch
    c = _calib(w, h, source)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=3) as eng, eng.rectifier(c) as r:
        info = r.info
        assert (info["src_w"], info["src_h"], info["w"], info["h"]) == (c.src_w, c.src_h, w, h)
        assert [info["valid_left"], info["valid_right"]] == [int((~rectify.is_sentinel(m)).sum()) for m in _maps(w, h, source)]
        for n in (1, 3):
            src, want, want_ten = _case(w, h, source, n)
            # host mode, side by side at pitch 2 sw + 16
            sbs, ten = r.rectify(src, None, src.shape[2], n, want_tensor=True)
            print(f"{source} -> {w}x{h} n={n}: host differing bytes {int((sbs != want).sum())} (frame), {int((ten != want_ten).sum())} (tensor)")
            assert np.array_equal(sbs, want) and np.array_equal(ten, want_ten)
            if source == "identity":                                             # the raw frame itself
                assert np.array_equal(sbs, src[:, :, :2 * w])
            for separate in (False, True):
                dsbs, dten = _device_call(torch, r, c, src, n, w, h, separate)
                assert np.array_equal(dsbs, want) and np.array_equal(dten, want_ten), (n, separate)
            # the tensor alone goes through the object's scratch; the frame alone writes no tensor
            _, only_ten = _device_call(torch, r, c, src, n, w, h, True, want_sbs=False)
            assert np.array_equal(only_ten, want_ten)
            assert np.array_equal(r.rectify(src, None, src.shape[2], n, want_sbs=False, want_tensor=True), want_ten)
            # ... and equals the library's own pre-processing of the rectified frame
            assert np.array_equal(eng.preprocess_sbs_nv12(want.reshape(n, -1)), want_ten)


@pytest.mark.gpu
def test_rectify_full_size(model_factory):
    import torch
    w, h, n = 1280, 720, 2
    c = rectify.synthetic_rig(1920, 1080, w, h, 1920)
    maps = tuple(rectify.build_map(c, eye, w, h) for eye in (0, 1))
    for m in maps:
        nv = rectify.nonvacuity(m, 1920, 1080)
        assert 0.01 < nv["sentinels"] < 0.50 and nv["partly_outside"] >= 1 and nv["both_fractions"] > 0.90, nv
    src = _sbs_source(1920, 1080, n, 2 * 1920, 9)
    want = rectify.reference(c, w, h, src, None, 2 * 1920, n, maps=maps)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n) as eng, eng.rectifier(c) as r:
        for eye in (0, 1):
            assert np.array_equal(r.map(eye), maps[eye])
        sbs, ten = _device_call(torch, r, c, src, n, w, h, False)
        print(f"1920x1080 -> 1280x720 n={n}: differing bytes {int((sbs != want).sum())}")
        assert np.array_equal(sbs, want) and np.array_equal(ten, rectify.tensor_from_sbs(want))


@pytest.mark.gpu
def test_rectify_map_and_call_forms_agree(model_factory):
    import torch
    w, h, source, n = 132, 70, "160x120", 3
    c = _calib(w, h, source)
    src, want, want_ten = _case(w, h, source, n)
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=n) as eng, eng.rectifier(c) as r:
        for eye in (0, 1):                                                        # the device copy is the host builder's map
            assert np.array_equal(r.map(eye), api.rectify_build_map(c, eye, w, h))
            assert np.array_equal(r.map(eye), _maps(w, h, source)[eye])
        host = r.rectify(src, None, src.shape[2], n, want_tensor=True)
        again = r.rectify(src, None, src.shape[2], n, want_tensor=True)          # two runs are identical
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, again))
        singles = [r.rectify(src[k], None, src.shape[2], 1, want_tensor=True) for k in range(n)]      # a batch = n single calls
        assert np.array_equal(np.concatenate([s[0] for s in singles]), host[0])
        assert np.array_equal(np.concatenate([s[1] for s in singles]), host[1])
        own = _device_call(torch, r, c, src, n, w, h, False)                     # device mode, the rectifier's own stream
        s1 = torch.cuda.Stream()
        theirs = _device_call(torch, r, c, src, n, w, h, False, stream=s1.cuda_stream)      # ... and a caller's stream
        for got in (own, theirs):
            assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
        assert np.array_equal(host[0], want) and np.array_equal(host[1], want_ten)
        cam = r.camera
        assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline_mm) == tuple(
            float(np.float32(v)) for v in (c.pfx, c.pfy, c.pcx, c.pcy, c.baseline_mm))
        assert (cam.z_min_m, cam.z_max_m, cam.step) == (0.0, 0.0, 1)


@pytest.mark.gpu
def test_rectified_frame_composes_with_inference_and_the_point_cloud(model_factory):
    w, h, d = 96, 64, 48
    with api.StereoNetHIP(model_factory(w, h, d), precision=api.PREC_F16) as eng:
        # a raw 128x80 pair -> rectified frame and tensor: the two inference entry points agree on them
        c = _calib(w, h, "128x80")
        src, want, _ = _case(w, h, "128x80", 1)
        with eng.rectifier(c) as r:
            sbs, ten = r.rectify(src, None, src.shape[2], 1, want_tensor=True)
            cam = r.camera
        assert np.array_equal(sbs, want)
        disp_a, raw_a = eng.infer_sbs_nv12(sbs[0])
        disp_b, raw_b = eng.infer(ten[0])
        assert np.array_equal(raw_a, raw_b) and np.array_equal(disp_a.view(np.uint32), disp_b.view(np.uint32))
        # the rectifier's camera feeds the point cloud: Z is sn_depth_from_raw's depth with fx
        pts, _ = eng.pointcloud(raw_a, cam)
        depth = eng.depth_from_raw(raw_a, cam.fx, cam.baseline_mm)
        valid = raw_a > 0
        assert valid.any() and np.array_equal(pts[..., 2][valid].view(np.uint32), depth[valid].view(np.uint32))
        # the identity calibration: all of it equals inference on the raw frame
        frame = synth.sbs_nv12_frame(w, h, d, 31).reshape(h * 3 // 2, 2 * w)
        with eng.rectifier(rectify.identity(w, h)) as r:
            sbs, ten = r.rectify(frame, want_tensor=True)
        assert np.array_equal(sbs[0], frame)
        disp_0, raw_0 = eng.infer_sbs_nv12(frame)
        disp_1, raw_1 = eng.infer_sbs_nv12(sbs[0])
        disp_2, raw_2 = eng.infer(ten[0])
        assert np.array_equal(raw_0, raw_1) and np.array_equal(raw_0, raw_2) and len(np.unique(raw_0)) > 16
        assert np.array_equal(disp_0.view(np.uint32), disp_1.view(np.uint32)) and np.array_equal(disp_0.view(np.uint32), disp_2.view(np.uint32))


@pytest.mark.gpu
def test_rectify_argument_errors_and_destroy_order(model_factory):
    import torch
    w, h, source = 96, 64, "128x80"
    c = _calib(w, h, source)
    src, want, want_ten = _case(w, h, source, 1)
    sw, sh = c.src_w, c.src_h
    pitch, rows = src.shape[2], sh + sh // 2
    # a model whose frames the side-by-side entry points cannot take either
    with api.StereoNetHIP(model_factory(1242, 375, 256)) as odd:                  # W % 4 == 2, and an odd height
        t = C.c_void_p()
        assert odd._lib.sn_rectify_create(odd._h, C.byref(api.stereo_calib(c)), C.byref(t)) == -1 and not t.value
        assert "sn_rectify_create" in odd._lib.sn_last_error(odd._h).decode() and "multiple of 4" in odd._lib.sn_last_error(odd._h).decode()
    eng = api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=2, precision=api.PREC_F16)
    lib, hd = eng._lib, eng._h

    def failed(rc, name):
        return rc == -1 and name in lib.sn_last_error(hd).decode()

    t = C.c_void_p()
    nan_d = dataclasses.replace(c, left=dataclasses.replace(c.left, d=(float("nan"), 0, 0, 0, 0)))
    bad = [lib.sn_rectify_create(hd, None, C.byref(t)), lib.sn_rectify_create(hd, C.byref(api.stereo_calib(c)), None),
           lib.sn_rectify_create(hd, C.byref(api.stereo_calib(nan_d)), C.byref(t)),
           lib.sn_rectify_create(hd, C.byref(api.stereo_calib(dataclasses.replace(c, src_w=127))), C.byref(t)),
           lib.sn_rectify_create(hd, C.byref(api.stereo_calib(dataclasses.replace(c, baseline_mm=0.0))), C.byref(t))]
    assert all(failed(rc, "sn_rectify_create") for rc in bad) and not t.value, bad
    r = eng.rectifier(c)
    flat = np.ascontiguousarray(src).reshape(-1)
    two = np.concatenate([flat, flat])
    out = np.full((2, h * 3 // 2, 2 * w), 0x11, np.uint8)
    ten = np.full((2, 6, h, w), 0x11, np.int8)

    def call(n=1, l=flat, rgt=None, p=pitch, f=pitch * rows, o=out, tn=None, mem=api.SN_MEM_HOST):
        ptr = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data      # noqa: E731
        rp = ptr(l) + sw if rgt is None and l is not None else ptr(rgt)
        return lib.sn_rectify_nv12(r._r, n, ptr(l), rp, p, f, ptr(o), ptr(tn), mem, None)

    bad = [call(n=0), call(n=-1), call(n=3, l=two), call(l=None, rgt=flat), call(o=None, tn=None), call(p=sw - 2), call(p=2 ** 30),
           call(mem=2)]
    assert all(failed(rc, "sn_rectify_nv12") for rc in bad), bad
    assert lib.sn_rectify_nv12(r._r, 1, flat.ctypes.data, None, pitch, pitch * rows, out.ctypes.data, None, 0, None) == -1
    # overlap: an output inside an input span, an input inside an output, the tensor on the last four bytes of the right eye's
    # span (which ends 16 bytes before the frame does: the pitch is 2 sw + 16), the two outputs on each other
    big = np.zeros(flat.size + out.size + ten.size, np.uint8)
    over = [call(l=big, o=big[8:].ctypes.data), call(l=big[out[0].size - 8:], o=big.ctypes.data),
            call(l=big, tn=big[flat.size - 20:].ctypes.data, o=None), call(o=big.ctypes.data, tn=big[out[0].size - 4:].ctypes.data)]
    assert all(failed(rc, "sn_rectify_nv12") for rc in over), over
    assert "overlap" in lib.sn_last_error(hd).decode()
    # device mode: outputs must be 4-byte aligned
    d_src = torch.from_numpy(flat).cuda()
    d_out = torch.zeros(out[0].size + 8, dtype=torch.uint8, device="cuda")
    d_ten = torch.zeros(ten[0].size + 8, dtype=torch.uint8, device="cuda")
    for so, st_ in ((1, 0), (2, 0), (0, 2), (0, 3)):
        rc = lib.sn_rectify_nv12(r._r, 1, d_src.data_ptr(), d_src.data_ptr() + sw, pitch, pitch * rows, d_out.data_ptr() + so,
                                 d_ten.data_ptr() + st_, api.SN_MEM_DEVICE, None)
        assert failed(rc, "sn_rectify_nv12") and "aligned" in lib.sn_last_error(hd).decode()
    assert failed(lib.sn_rectify_get_map(r._r, 2, out.ctypes.data), "sn_rectify_get_map")
    assert failed(lib.sn_rectify_get_map(r._r, 0, None), "sn_rectify_get_map")
    assert lib.sn_rectify_get_info(r._r, None) == -1 and lib.sn_rectify_get_camera(None, None) == -1
    with pytest.raises(api.StereoNetError):
        r.rectify(flat[:flat.size // 2], None, pitch)                           # a buffer too short for one frame
    # nothing was written by any failed call, and a valid call still gives the right answer
    assert np.all(out == 0x11) and np.all(ten == 0x11) and not d_out.any() and not d_ten.any()
    assert call(tn=ten) == 0 and np.array_equal(out[0], want[0]) and np.array_equal(ten[0], want_ten[0])
    assert np.all(out[1] == 0x11) and np.all(ten[1] == 0x11)
    # destroying the handle under a live rectifier is refused and leaves both usable
    assert lib.sn_destroy(hd) == -6 and "rectif" in lib.sn_last_error(hd).decode()
    with pytest.raises(api.StereoNetError):
        eng.close()
    out[:] = 0
    assert call() == 0 and np.array_equal(out[0], want[0])
    r.close()
    eng.close()
    assert not eng._h.value


def _write_raw_lists(tmp_path, sw, sh, n):
    from hobot_stereonet_amd import images
    rng = np.random.default_rng(17)
    names = {"l": [], "r": []}
    for k in range(n):
        base = rng.integers(0, 256, (sh // 8, sw // 8, 3)).astype(np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))                         # blocks, so that the eyes have structure
        for side, shift in (("l", 0), ("r", 3)):
            eye = np.clip(np.roll(img, -shift, 1).astype(np.int16) + rng.integers(-4, 5, img.shape), 0, 255).astype(np.uint8)
            p = str(tmp_path / f"{side}{k}.png")
            images.write_png(p, eye)
            names[side].append(p)
    for side in ("l", "r"):
        (tmp_path / f"{side}.list").write_text("".join(f"{p}\n" for p in names[side]))
    return names


@pytest.mark.gpu
def test_filelist_rectify(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    w, h, d, n = 96, 64, 48, 2
    model = model_factory(w, h, d)
    c = _calib(w, h, "128x80")
    rectify.save_calib(str(tmp_path / "calib.txt"), c)
    names = _write_raw_lists(tmp_path, 128, 80, n)
    base = ["--model", model, "--left", str(tmp_path / "l.list"), "--right", str(tmp_path / "r.list"), "--precision", "f16"]
    capsys.readouterr()
    assert filelist.main(base + ["--out", str(tmp_path / "o"), "--rectify", str(tmp_path / "calib.txt"), "--ply", str(tmp_path / "p")]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    maps = _maps(w, h, "128x80")
    assert summary["frames"] == n and [summary["valid_left"], summary["valid_right"]] == [int((~rectify.is_sentinel(m)).sum()) for m in maps]
    assert sorted(os.listdir(tmp_path / "o")) == sorted(f"{i}.{e}" for i in range(n) for e in ("raw.bin", "disp.pfm", "depth.ppm", "rect.ppm"))
    assert sorted(os.listdir(tmp_path / "p")) == [f"{i}.ply" for i in range(n)]
    with api.StereoNetHIP(model, precision=api.PREC_F16) as eng:
        for i in range(n):
            eyes = [images.bgr_to_nv12(images.imread_bgr(names[s][i])) for s in ("l", "r")]
            want = rectify.reference(c, w, h, eyes[0], eyes[1], maps=maps)[0]
            assert np.array_equal(images.read_pnm(str(tmp_path / "o" / f"{i}.rect.ppm")), rectify.sbs_to_rgb(want))
            assert open(tmp_path / "o" / f"{i}.raw.bin", "rb").read() == eng.infer_sbs_nv12(want)[1].tobytes()
    # the identity calibration on model-size images: the disparity outputs are those of a run without --rectify
    names = _write_raw_lists(tmp_path, w, h, n)
    rectify.save_calib(str(tmp_path / "id.txt"), rectify.identity(w, h))
    assert filelist.main(base + ["--out", str(tmp_path / "a")]) == 0
    assert filelist.main(base + ["--out", str(tmp_path / "b"), "--rectify", str(tmp_path / "id.txt")]) == 0
    for i in range(n):
        for e in ("raw.bin", "disp.pfm", "depth.ppm"):
            assert open(tmp_path / "a" / f"{i}.{e}", "rb").read() == open(tmp_path / "b" / f"{i}.{e}", "rb").read(), (i, e)
    # raw images of another size than the calibration's are refused, as a wrong size is without it
    assert filelist.main(base + ["--rectify", str(tmp_path / "calib.txt")]) == 5
    with pytest.raises(SystemExit):
        filelist.main(base + ["--rectify", str(tmp_path / "missing.txt")])


def _payloads(prefix, n, w, h):
    return [open(f"{prefix}.{i}.msg", "rb").read() for i in range(n)]


@pytest.mark.gpu
def test_node_rectifies_raw_frames(model_factory, tmp_path):
    import subprocess
    compat = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc", "compat")
    subprocess.check_call(["make", "-C", compat, "-s"])
    exe = os.path.join(compat, "build", "rectify_harness")
    w, h, d, n = 96, 64, 48, 2
    model = model_factory(w, h, d)
    env = {k: v for k, v in os.environ.items() if not k.startswith("STEREONET_RECTIFY")}
    env["STEREONET_PRECISION"] = "fp32"             # pinned: the default's first-call calibration is not a function of the frame

    def run(tag, frames, sw, sh, calib=None):
        frames.tofile(str(tmp_path / f"{tag}.bin"))
        e = env
        if calib is not None:
            rectify.save_calib(str(tmp_path / f"{tag}.txt"), calib)
            e = dict(env, STEREONET_RECTIFY=str(tmp_path / f"{tag}.txt"))
        r = subprocess.run([exe, model, str(tmp_path / f"{tag}.bin"), str(sw), str(sh), str(n), str(tmp_path / tag)],
                           capture_output=True, text=True, env=e, timeout=120)
        assert r.returncode == 0 and f"received={n}" in r.stdout, r.stderr[-2000:]
        return r, _payloads(tmp_path / tag, n, w, h)

    # the identity calibration on frames of the model's size: the messages are those of a node without the variable
    plain_frames = np.stack([synth.sbs_nv12_frame(w, h, d, 40 + k).reshape(h * 3 // 2, 2 * w) for k in range(n)])
    off, plain = run("off", plain_frames, w, h)
    on, same = run("id", plain_frames, w, h, rectify.identity(w, h))
    assert "rectification:" in on.stderr and "rectification" not in off.stderr
    assert same == plain and len(plain[0]) > 4 * w * h and plain[0] != plain[1]
    # raw 128x80 frames: the int32 part is inference on the twin's rectified frame
    c = _calib(w, h, "128x80")
    raw = _sbs_source(128, 80, n, 2 * 128, 77)
    rect, got = run("raw", raw, 128, 80, c)
    want = rectify.reference(c, w, h, raw, None, 2 * 128, n, maps=_maps(w, h, "128x80"))
    with api.StereoNetHIP(model, precision=api.PREC_FP32) as eng:
        for k in range(n):
            assert got[k][:4 * w * h] == eng.infer_sbs_nv12(want[k])[1].tobytes(), k
            assert len(got[k]) > 4 * w * h                                       # the JPEG of the rectified left eye follows
    # a file that cannot be read turns rectification off with one error line: the node is the one without the variable
    (tmp_path / "bad.txt").write_text("size 96 64\nleft.K 1 1 0\n")
    r = subprocess.run([exe, model, str(tmp_path / "off.bin"), str(w), str(h), str(n), str(tmp_path / "bad")], capture_output=True,
                       text=True, env=dict(env, STEREONET_RECTIFY=str(tmp_path / "bad.txt")), timeout=120)
    assert r.returncode == 0 and r.stderr.count("no rectification") == 1, r.stderr[-2000:]
    assert _payloads(tmp_path / "bad", n, w, h) == plain
