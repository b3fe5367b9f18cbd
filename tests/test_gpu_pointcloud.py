"""sn_pointcloud_from_raw on the MI355X: the kernels equal the numpy twin (hobot_stereonet_amd/pointcloud.py) bit for bit,
Z equals sn_depth_from_raw, device mode on two torch streams equals host mode, the cloud of a real inference, the call
beside sn_submit / sn_wait, and the node's /stereonet_pointcloud2 topic."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from hobot_stereonet_amd import api, pointcloud, synth
from hobot_stereonet_amd.pointcloud import COMPACT, ORGANISED, Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
D = {(96, 64): 48, (1242, 375): 256, (1280, 720): 192}


def _raw(n, w, h, seed):
    """int32 maps with ~70 % valid samples, and the corner values 0, 1, 200000, 2^31 - 1."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(1, 600000, (n, h, w)).astype(np.int32)
    raw[rng.random((n, h, w)) < 0.3] = 0
    raw[0, 0, :4] = [0, 1, 200000, 2 ** 31 - 1]
    raw[-1, -1, -3:] = [-7, 2 ** 31 - 1, 1]
    return raw


def _nv12(n, pitch, h, seed):
    return np.random.default_rng(seed).integers(0, 256, n * pointcloud.nv12_frame_bytes(pitch, h), dtype=np.uint8)


def _same(got, want, counts, layout):
    if layout == ORGANISED:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return all(np.array_equal(got[k, :c].view(np.uint32), want[k, :c].view(np.uint32)) for k, c in enumerate(counts))


def _grid(w, h):
    """(n, step, camera, colour pitch multiple or None): every combination at the small shape; at the large ones a set
    that still covers every axis (n, step, camera, colour at pitch W and 2W) and keeps the file inside its time budget."""
    cams = [Camera(), Camera(fx=600.5, fy=590.25, cx=w / 2 - 3.3, cy=h / 2 + 1.7, z_min_m=0.3, z_max_m=2.0)]
    if (w, h) == (96, 64):
        return [(n, s, c, col) for n in (1, 3) for s in (1, 2, 4) for c in cams for col in (None, 1, 2)]
    return [(1, 1, cams[0], None), (3, 1, cams[1], 2), (1, 2, cams[1], 1), (3, 4, cams[0], None), (1, 1, cams[0], 1),
            (3, 2, cams[0], 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(96, 64), (1242, 375), (1280, 720)])
def test_kernels_equal_twin_bit_for_bit(model_factory, w, h):
    raws = {n: _raw(n, w, h, n + w) for n in (1, 3)}
    with api.StereoNetHIP(model_factory(w, h, D[(w, h)]), max_batch=3) as eng:
        for n, step, cam0, colour in _grid(w, h):
            cam = Camera(**{**cam0.__dict__, "step": step})
            pitch = colour * w if colour else 0
            nv12 = _nv12(n, pitch, h, 7) if colour else None
            for layout in (ORGANISED, COMPACT):
                got, gc = eng.pointcloud(raws[n], cam, layout, nv12, pitch)
                want, wc = pointcloud.reference(raws[n], cam, layout, nv12, pitch, eng.out_scale)
                tag = f"n={n} step={step} cam={cam} colour={colour} layout={layout}"
                assert np.array_equal(gc, wc), tag
                assert _same(got, want, wc, layout), tag


@pytest.mark.gpu
def test_z_equals_depth_from_raw_and_compact_equals_organised(model_factory):
    w, h = 1280, 720
    raw = _raw(2, w, h, 3)
    with api.StereoNetHIP(model_factory(w, h, 192), max_batch=2) as eng:
        depth = eng.depth_from_raw(raw)
        org, oc = eng.pointcloud(raw, Camera(), ORGANISED)
        cmp_, cc = eng.pointcloud(raw, Camera(), COMPACT)
    valid = raw > 0
    assert np.array_equal(org[..., 2][valid].view(np.uint32), depth[valid].view(np.uint32))
    assert np.array_equal(oc, cc) and oc.tolist() == valid.reshape(2, -1).sum(1).tolist()
    for k in range(2):
        assert np.array_equal(cmp_[k, :cc[k]].view(np.uint32), org[k][valid[k]].view(np.uint32))


@pytest.mark.gpu
def test_device_mode_two_streams_equals_host_mode(model_factory):
    import torch
    w, h, n = 1280, 720, 2
    raw = _raw(n, w, h, 11)
    nv12 = _nv12(n, 2 * w, h, 12)
    cam = Camera(step=2, z_max_m=3.0)
    ho, wo = cam.out_shape(w, h)
    with api.StereoNetHIP(model_factory(w, h, 192), max_batch=n) as eng:
        want_c, want_cc = eng.pointcloud(raw, cam, COMPACT, nv12, 2 * w)
        want_o, want_oc = eng.pointcloud(raw, Camera(), ORGANISED)
        draw = torch.from_numpy(raw).cuda()
        dnv = torch.from_numpy(nv12).cuda()
        pc = torch.empty((n, ho * wo, 4), dtype=torch.float32, device="cuda")
        cc = torch.empty(n, dtype=torch.int32, device="cuda")
        po = torch.empty((n, h, w, 4), dtype=torch.float32, device="cuda")
        oc = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        eng.pointcloud_device(n, draw.data_ptr(), cam, pc.data_ptr(), cc.data_ptr(), dnv.data_ptr(), 2 * w, COMPACT,
                              s1.cuda_stream)
        eng.pointcloud_device(n, draw.data_ptr(), Camera(), po.data_ptr(), oc.data_ptr(), 0, 0, ORGANISED, s2.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        got_cc = cc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_cc, want_cc) and np.array_equal(oc.cpu().numpy().view(np.uint32), want_oc)
        assert _same(pc.cpu().numpy(), want_c, want_cc, COMPACT)
        assert np.array_equal(po.cpu().numpy().view(np.uint32), want_o.view(np.uint32))
        # NULL stream: the point cloud's own stream, returns after completion
        po.fill_(0)
        torch.cuda.synchronize()
        eng.pointcloud_device(n, draw.data_ptr(), Camera(), po.data_ptr(), 0)
        assert np.array_equal(po.cpu().numpy().view(np.uint32), want_o.view(np.uint32))


@pytest.mark.gpu
def test_compact_calls_on_two_streams_share_the_scratch_in_order(model_factory):
    """Two compact calls enqueued back to back on different streams use the one tile-count scratch with different tile
    counts (step 1: 225 tiles a map, step 2: 57): the event between them keeps the second call's count pass from
    overwriting the first call's counts before its write pass has read them."""
    import torch
    w, h, n = 1280, 720, 3
    raw_a, raw_b = _raw(n, w, h, 21), _raw(n, w, h, 22)
    cam_a, cam_b = Camera(z_max_m=4.0), Camera(step=2, z_min_m=0.4)
    with api.StereoNetHIP(model_factory(w, h, 192), max_batch=n) as eng:
        want = [pointcloud.reference(r, c, COMPACT, None, 0, eng.out_scale) for r, c in ((raw_a, cam_a), (raw_b, cam_b))]
        draws = [torch.from_numpy(r).cuda() for r in (raw_a, raw_b)]
        pts = [torch.empty((n, np.prod(c.out_shape(w, h)), 4), dtype=torch.float32, device="cuda") for c in (cam_a, cam_b)]
        cnts = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for rep in range(3):
            for k, cam in enumerate((cam_a, cam_b)):
                eng.pointcloud_device(n, draws[k].data_ptr(), cam, pts[k].data_ptr(), cnts[k].data_ptr(), 0, 0, COMPACT,
                                      streams[k].cuda_stream)
            for st in streams:
                st.synchronize()
            for k in range(2):
                wp, wc = want[k]
                got_c = cnts[k].cpu().numpy().view(np.uint32)
                assert np.array_equal(got_c, wc), (rep, k)
                assert _same(pts[k].cpu().numpy(), wp, wc, COMPACT), (rep, k)


@pytest.mark.gpu
def test_cloud_of_an_inference_host_and_device(model_factory):
    import torch
    w, h, d = 1280, 720, 192
    x = synth.model_input_i8(w, h, d, 5)
    l, _ = synth.stereo_pair_u8(w, h, d, 5)
    # the left eye as a plain NV12 image (pitch W): its luma plane, chroma from its "U" / "V" planes subsampled 2x2
    uv = np.stack([l[1][::2, ::2], l[2][::2, ::2]], -1).reshape(h // 2, w)
    nv12 = np.concatenate([l[0], uv], 0).ravel()
    cam = Camera(z_min_m=0.1, z_max_m=50.0)
    with api.StereoNetHIP(model_factory(w, h, d)) as eng:
        _, raw = eng.infer(x)
        want, wc = pointcloud.reference(raw, cam, COMPACT, nv12, w, eng.out_scale)
        got, gc = eng.pointcloud(raw, cam, COMPACT, nv12, w)
        assert gc[0] > 0 and np.array_equal(gc, wc) and _same(got[None], want[None], wc, COMPACT)
        draw = torch.from_numpy(raw).cuda()
        dnv = torch.from_numpy(nv12).cuda()
        po = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        oc = torch.empty(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.pointcloud_device(1, draw.data_ptr(), cam, po.data_ptr(), oc.data_ptr(), dnv.data_ptr(), w, ORGANISED)
        wo_, woc = pointcloud.reference(raw, cam, ORGANISED, nv12, w, eng.out_scale)
        assert np.array_equal(po.cpu().numpy().view(np.uint32), wo_.view(np.uint32)) and int(oc[0]) == int(woc[0])


@pytest.mark.gpu
def test_pointcloud_beside_submit_and_wait(model_factory):
    """4 sn_submit tickets in flight while another thread calls pointcloud (ctypes drops the GIL): every map equals the
    serial run, no ticket deadlocks."""
    w, h, d = 96, 64, 48
    xs = [synth.model_input_i8(w, h, d, s) for s in range(4)]
    rng = np.random.default_rng(9)
    craw = rng.integers(0, 400000, (h, w)).astype(np.int32)
    with api.StereoNetHIP(model_factory(w, h, d), task_num=4) as eng:
        serial = [eng.infer(x)[1] for x in xs]
        cref, ccnt = eng.pointcloud(craw, Camera(), COMPACT)
        errors, stop = [], threading.Event()

        def clouds():
            try:
                while not stop.is_set():
                    p, c = eng.pointcloud(craw, Camera(), COMPACT)
                    if not (np.array_equal(c, ccnt) and _same(p[None], cref[None], ccnt, COMPACT)):
                        errors.append("cloud differs")
            except Exception as e:        # noqa: BLE001
                errors.append(repr(e))

        t = threading.Thread(target=clouds)
        t0 = time.time()
        t.start()
        try:
            for _ in range(5):
                outs = [np.empty((h, w), np.int32) for _ in xs]
                tickets = [eng.submit(x, o, None) for x, o in zip(xs, outs)]
                for tk in tickets:
                    eng.wait(tk)
                for o, s in zip(outs, serial):
                    assert np.array_equal(o, s)
        finally:
            stop.set()
            t.join(30)
        assert not t.is_alive() and not errors, errors
        assert time.time() - t0 < 60


def _frames(sbs, w, n):
    out = []
    for i in range(n):
        f = sbs.copy()
        f[0:w:7] ^= np.uint8((i * 5) & 255)
        out.append(f)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["compact", "organised"])
def test_node_publishes_pointcloud2(model_factory, tmp_path, layout):
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    w, h, d = 96, 64, 48
    m = model_factory(w, h, d)
    lt, rt = synth.stereo_pair_u8(w, h, d, 8)
    frame = np.random.default_rng(8).integers(0, 256, (h * 3 // 2, 2 * w), dtype=np.uint8)
    frame[:h, :w] = lt[0]
    frame[:h, w:] = rt[0]
    sbs = frame.ravel()
    sbs.tofile(str(tmp_path / "s.bin"))
    nframes = 3
    exe = os.path.join(COMPAT, "build", "pointcloud_harness")
    base_env = {k: v for k, v in os.environ.items() if not k.startswith("STEREONET_POINTCLOUD")}
    base_env["STEREONET_PRECISION"] = "fp32"
    r0 = subprocess.run([exe, m, str(tmp_path / "s.bin"), str(w), str(h), str(nframes), str(tmp_path / "off")],
                        capture_output=True, text=True, env=base_env, timeout=120)
    assert r0.returncode == 0, r0.stderr
    assert "cloud " not in r0.stdout and f"received={nframes} clouds=0" in r0.stdout
    # settings the call would reject turn the cloud off at start-up with one error, not one per frame
    for bad in ({"STEREONET_POINTCLOUD_STEP": "3"}, {"STEREONET_CAMERA": "0,500,48,32,120"},
                {"STEREONET_POINTCLOUD_Z": "near,far"}):
        rb = subprocess.run([exe, m, str(tmp_path / "s.bin"), str(w), str(h), str(nframes), str(tmp_path / "bad")],
                            capture_output=True, text=True, env=dict(base_env, STEREONET_POINTCLOUD=layout, **bad),
                            timeout=120)
        assert rb.returncode == 0, rb.stderr
        assert f"received={nframes} clouds=0" in rb.stdout, bad
        assert rb.stderr.count("no point cloud") == 1 and "point cloud failed" not in rb.stderr, (bad, rb.stderr[-2000:])
    env = dict(base_env, STEREONET_POINTCLOUD=layout, STEREONET_POINTCLOUD_Z="0.05,0")
    r = subprocess.run([exe, m, str(tmp_path / "s.bin"), str(w), str(h), str(nframes), str(tmp_path / "on")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("cloud ")]
    assert len(lines) == nframes
    frames = _frames(sbs, w, nframes)
    cam = Camera(z_min_m=0.05)
    for i, line in enumerate(lines):
        meta = dict(kv.split("=", 1) for kv in line.split()[1:])
        off = open(tmp_path / f"off.{i}.msg", "rb").read()
        on = open(tmp_path / f"on.{i}.msg", "rb").read()
        assert on == off                                      # the disparity message is untouched by the cloud
        assert meta["frame_id"] == str(100 + i) and meta["stamp"] == f"7.{1000 + i}"
        assert meta["fields"] == "x:0:7:1,y:4:7:1,z:8:7:1,rgb:12:7:1"
        assert meta["point_step"] == "16" and meta["is_bigendian"] == "0"
        raw = np.frombuffer(on[:w * h * 4], np.int32).reshape(h, w)
        lay = COMPACT if layout == "compact" else ORGANISED
        want, wc = pointcloud.reference(raw, cam, lay, frames[i], 2 * w)
        data = np.fromfile(str(tmp_path / f"on.{i}.pc"), np.uint32)
        if lay == COMPACT:
            assert meta["height"] == "1" and meta["width"] == str(wc[0]) and meta["is_dense"] == "1"
            assert np.array_equal(data, want[:wc[0]].view(np.uint32).ravel())
        else:
            assert meta["height"] == str(h) and meta["width"] == str(w) and meta["is_dense"] == "0"
            assert np.array_equal(data, want.view(np.uint32).ravel())
        assert meta["row_step"] == str(16 * int(meta["width"]))
        assert int(meta["len"]) == int(meta["row_step"]) * int(meta["height"])


@pytest.mark.gpu
def test_filelist_ply(model_factory, tmp_path):
    """filelist --ply DIR --camera ...: one PLY per pair, the compact cloud of the pair's map coloured by its left eye."""
    from hobot_stereonet_amd import filelist, images
    w, h, d = 96, 64, 48
    lt, rt = synth.stereo_pair_u8(w, h, d, 4)
    paths = []
    for name, eye in (("l.ppm", lt), ("r.ppm", rt)):
        rgb = np.repeat(eye[0][..., None], 3, -1)
        images.write_ppm(str(tmp_path / name), rgb)
        paths.append(str(tmp_path / name))
    for side, p in zip("lr", paths):
        (tmp_path / f"{side}.list").write_text(f"{p}\n{p}\n")
    out = tmp_path / "ply"
    rc = filelist.main(["--model", model_factory(w, h, d), "--left", str(tmp_path / "l.list"), "--right",
                        str(tmp_path / "r.list"), "--ply", str(out), "--camera", "500,500,48,32,120"])
    assert rc == 0 and sorted(os.listdir(out)) == ["0.ply", "1.ply"]
    cam = Camera(fx=500.0, fy=500.0, cx=48.0, cy=32.0, baseline_mm=120.0)
    with api.StereoNetHIP(model_factory(w, h, d)) as eng:
        eyes = [images.bgr_to_nv12(images.imread_bgr(p)) for p in paths]
        sbs = images.sbs_from_eyes(eyes[0], eyes[1], w, h)
        _, raw = eng.infer_sbs_nv12(sbs)
    want, wc = pointcloud.reference(raw, cam, COMPACT, sbs, 2 * w)
    v = pointcloud.read_ply(str(out / "0.ply"))
    assert len(v) == wc[0] > 0
    assert np.array_equal(v["z"], want[:wc[0], 2]) and np.array_equal(v["x"], want[:wc[0], 0])
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), pointcloud.unpack_rgb(want[:wc[0]]))
