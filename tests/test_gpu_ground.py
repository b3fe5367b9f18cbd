"""sn_ground_from_raw and sn_obstacles_from_raw_mounts on the MI355X: the records (flags, counts, the Q16 plane, and the float
outputs as bits) and the labels equal the numpy twin's (hobot_stereonet_amd/ground.py) byte for byte on ten constructed maps,
for every step, hypothesis count, refit count and region, every combination of outputs, every call form, with guard bytes
untouched; a shape with W % 4 == 2 and an odd height; a batch against single calls; beside inference; the chain map -> ground
-> obstacles on one stream; argument errors; what sn_destroy leaves behind; the node's grid under the frame's mount and the
filelist tool.

No tolerance appears: the contract is the same bytes.  The twin is fed the library's gate (the two gates may differ by one where
cos and sin differ by an ulp, tests/test_ground.py)."""
import ctypes as C
import dataclasses
import functools
import itertools
import json
import math
import os
import subprocess
import threading

import numpy as np
import pytest

from hobot_stereonet_amd import api, ground, obstacles, synth, weights
from hobot_stereonet_amd.ground import GroundParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG = -1                    # SN_ERR_ARG (include/stereonet_hip.h)
REC = ground.RECORD.itemsize
CAM = Camera(fx=64.0, fy=64.0, cx=48.0, cy=32.0, baseline_mm=120.0)
PRIOR = obstacles.mount(0.0, 0.0, (0.1, -0.05, 0.5))
BASE = GroundParams(base_from_cam=PRIOR, hypotheses=64, seed=7, refits=2, tol_px=0.02, min_inliers=400, min_area=16, height_min_m=0.2,
                    height_max_m=2.0)
TOL = ground.tol_raw(BASE)      # 39
MOVED_IN, MOVED_OUT = ((40, 5), (50, 90), (63, 47)), ((41, 6), (51, 91), (62, 40), (33, 0))


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _planar(w=W, h=H, cam=CAM):
    """an exactly integer-planar map, raw = 3 (u - cx) + 480 (v - cy) + 200: the floor under a level camera at 0.5 m, nearly"""
    v, u = np.mgrid[0:h, 0:w]
    return (3 * (u - int(cam.cx)) + 480 * (v - int(cam.cy)) + 200).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _maps():
    """ten different maps, shared by the tests and never changed: 0 exactly planar (every live hypothesis counts every sample),
    1 the same with three pixels moved by exactly tol_raw and four by tol_raw + 1, 2 the same with pixels at 2^24 (a usable
    outlier) and 2^24 + 1 (not usable), 3 a level scene, 4 a pitched and rolled scene with a wall, boxes, outliers and holes,
    5 a scene whose wall holds more of the region than its floor, 6 zeros, 7 a constant (a wall: dies in the gate), 8 any int32
    word, 9 a floor of five rows under a wall (below min_inliers)"""
    rng = np.random.default_rng(9)
    raw = np.zeros((MAX_BATCH, H, W), np.int32)
    raw[0] = _planar()
    raw[1] = raw[0]
    for v, u in MOVED_IN:
        raw[1, v, u] += TOL if (u + v) & 1 else -TOL
    for v, u in MOVED_OUT:
        raw[1, v, u] += TOL + 1 if (u + v) & 1 else -(TOL + 1)
    raw[2] = raw[0]
    raw[2, 34:60:5, 3:90:7] = 1 << 24
    raw[2, 35:60:5, 4:90:7] = (1 << 24) + 1
    raw[3] = ground.scene(W, H, CAM, 0.5)[0]
    raw[4] = ground.scene(W, H, CAM, 0.7, 0.2, -0.1, wall_z_m=5.0, boxes=2, hole_frac=0.1, outlier_frac=0.15, seed=4)[0]
    raw[5] = ground.scene(W, H, CAM, 0.8, 0.1, 0.0, wall_z_m=2.0, outlier_frac=0.05, seed=5)[0]
    raw[7] = 9000
    raw[8] = rng.integers(-(1 << 31), 1 << 31, (H, W), dtype=np.int64).astype(np.int32)
    raw[9] = np.maximum(ground.scene(W, H, CAM, 0.5)[0], raw[0, 58, 48])
    raw.setflags(write=False)
    return raw


_TWINS = {}


def _twin(p=BASE, step=1):
    """the twin on the ten maps with the library's gate: (records, labels), computed once and read-only"""
    key = (dataclasses.astuple(p), step)
    if key not in _TWINS:
        c = dataclasses.replace(CAM, step=step)
        out = ground.reference(_maps(), c, p, gate_q16=api.ground_gate(c, p, W, H))
        for a in out:
            a.setflags(write=False)
        _TWINS[key] = out
    return _TWINS[key]


def _device(torch, e, raw, cam, p, want=(True, True), stream=0, shift=0):
    """device mode: every wanted output GUARD bytes into a buffer of 0x5a of its own, raw `shift` bytes into its buffer ->
    (records, labels) (None where not wanted), after checking every byte the call must not write"""
    n, h, w = raw.shape
    sizes = (n * REC, n * h * w)
    d_raw = torch.zeros(raw.size * 4 + shift + 16, dtype=torch.uint8, device="cuda")
    d_raw[shift:shift + raw.size * 4].copy_(torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1).copy()))
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(sizes, want)]
    torch.cuda.synchronize()
    e.ground_device(n, d_raw.data_ptr() + shift, cam, p, *[b.data_ptr() + GUARD if b is not None else 0 for b in bufs], stream=stream)
    if stream:
        torch.cuda.synchronize()
    parts = []
    for name, b, s in zip(("ground", "labels"), bufs, sizes):
        if b is None:
            parts.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a), f"guard bytes around {name}"
        parts.append(o[GUARD:GUARD + s].copy())
    return (None if parts[0] is None else parts[0].view(ground.RECORD), None if parts[1] is None else parts[1].reshape(n, h, w))


def _differing(got, want, n=None):
    """what differs from the twin's first n maps: the names of the record's fields (floats compared as bits), and `labels`"""
    bad = []
    rec, lab = got
    wrec, wlab = (want[0], want[1]) if n is None else (want[0][:n], want[1][:n])
    if rec is not None:
        rec = np.atleast_1d(rec)
        bad += [f for f in ground.RECORD.names if np.ascontiguousarray(rec[f]).tobytes() != np.ascontiguousarray(np.atleast_1d(wrec)[f]).tobytes()]
        if rec.tobytes() != np.atleast_1d(wrec).tobytes() and not bad:
            bad.append("record")
    if lab is not None and (lab.shape != wlab.shape or not np.array_equal(lab, wlab)):
        bad.append("labels")
    return bad


@pytest.mark.gpu
def test_bytes_equal_twin_on_the_ten_maps_and_every_step(eng):
    import torch
    raw = _maps()
    bad = []
    for step in (1, 2, 4):
        p = dataclasses.replace(BASE, min_inliers=BASE.min_inliers // (step * step))
        for shift in (0, 4):                            # a map base that is 4- but not 16-byte aligned: the scalar label pass
            got = _device(torch, eng, raw, dataclasses.replace(CAM, step=step), p, shift=shift)
            if _differing(got, _twin(p, step)):
                bad.append((step, shift, _differing(got, _twin(p, step))))
    assert not bad, bad
    # the inputs do what they were built for
    rec, lab = _twin()
    fl = [int(f) & ~ground.SINGULAR for f in rec["flags"]]
    assert fl[:6] == [ground.FOUND] * 6 and fl[6] == fl[7] == fl[8] == ground.NO_HYPOTHESIS and fl[9] == ground.FEW_INLIERS, fl
    assert rec["usable"][0] == rec["inliers"][0] == 96 * 32 and tuple(rec["plane_q16"][0]) == (3 * 65536, 480 * 65536, 200 * 65536 + 16 * 480 * 65536)
    assert rec["survivors"][0] > 8 and rec["winner"][0] == min(i for i in range(BASE.hypotheses) if _live(i))      # the lowest live index of a tie
    assert rec["usable"][2] == rec["usable"][0] - np.count_nonzero(_maps()[2, 32:] == (1 << 24) + 1) and rec["inliers"][2] < rec["usable"][2]
    assert rec["usable"][6] == 0 and rec["usable"][7] == 96 * 32 and rec["survivors"][7] == 0 and 0 < rec["inliers"][9] < BASE.min_inliers
    assert abs(rec["plane_cam"][4][3] - 0.7) < 3e-3 and abs(rec["plane_cam"][5][3] - 0.8) < 3e-3 and abs(rec["base_from_cam"][3][11] - 0.5) < 1e-4
    assert np.array_equal(rec["base_from_cam"][9], np.float32(PRIOR)) and np.array_equal(rec["base_from_cam"][3][[3, 7]], np.float32(PRIOR)[[3, 7]])
    assert {1, 2, 3} <= set(np.unique(lab[4])) and np.all(lab[6] == 0) and np.all(lab[7] == 4) and set(np.unique(lab[8])) == {0, 4}


def _live(i):
    """hypothesis i of BASE on the planar map: its three samples span a triangle of the area asked for"""
    u, v = ground.sample_positions(BASE, ground.roi(BASE, W, H, 1), 1)
    return abs((u[i, 1] - u[i, 0]) * (v[i, 2] - v[i, 0]) - (v[i, 1] - v[i, 0]) * (u[i, 2] - u[i, 0])) >= BASE.min_area


@pytest.mark.gpu
def test_pixels_exactly_on_and_one_beyond_the_tolerance(eng):
    """without a refit the winner's plane is the planar map's own: a pixel moved by tol_raw stays an inlier and ground, one moved
    by tol_raw + 1 is neither"""
    import torch
    p = dataclasses.replace(BASE, refits=0)
    rec, lab = _device(torch, eng, _maps()[:2], CAM, p)
    assert not _differing((rec, lab), _twin(p), 2)
    assert rec["inliers"][1] == rec["inliers"][0] - len(MOVED_OUT) == 96 * 32 - len(MOVED_OUT)
    assert all(lab[1][v, u] == ground.LABEL_GROUND for v, u in MOVED_IN)
    assert all(lab[1][v, u] == (ground.LABEL_ABOVE if (u + v) & 1 else ground.LABEL_BELOW) for v, u in MOVED_OUT)
    assert np.count_nonzero(lab[1][32:] != ground.LABEL_GROUND) == len(MOVED_OUT)


@pytest.mark.gpu
def test_parameter_sweeps(eng):
    import torch
    raw = _maps()
    sweeps = [dataclasses.replace(BASE, hypotheses=k) for k in (1, 65, 128, 129, 1024)]
    sweeps += [dataclasses.replace(BASE, refits=r) for r in (0, 1, 3, 4)]
    sweeps += [dataclasses.replace(BASE, seed=s, min_area=a, tol_px=t) for s, a, t in ((0, 0, 0.0), (0xFFFFFFFF, 2000, 0.3), (123456, 1, 5.0))]
    sweeps += [dataclasses.replace(BASE, roi_x=0, roi_y=50, roi_w=W, roi_h=1),                  # one row: no triangle has an area
               dataclasses.replace(BASE, roi_x=10, roi_y=40, roi_w=3, roi_h=1),                 # three samples
               dataclasses.replace(BASE, roi_x=10, roi_y=40, roi_w=2, roi_h=2, min_area=1, min_inliers=3),
               dataclasses.replace(BASE, roi_x=5, roi_y=20, roi_w=70, roi_h=44, min_inliers=100),
               dataclasses.replace(BASE, roi_x=0, roi_y=0, roi_w=W, roi_h=H),
               dataclasses.replace(BASE, base_from_cam=(0.0,) * 12, max_tilt_rad=0.05),         # the all-zero prior; a narrow gate
               dataclasses.replace(BASE, base_from_cam=obstacles.mount(0.5, 0.15, (0.0, 0.3, 1.0)), max_tilt_rad=0.4, height_max_m=0.75)]
    bad = []
    for p, step in itertools.chain(((q, 1) for q in sweeps), ((sweeps[1], 2), (sweeps[4], 4), (sweeps[-4], 2), (sweeps[-1], 4))):
        got = _device(torch, eng, raw, dataclasses.replace(CAM, step=step), p)
        if _differing(got, _twin(p, step)):
            bad.append((p, step, _differing(got, _twin(p, step))))
    assert not bad, bad
    assert np.all(_twin(sweeps[-7])[0]["flags"] == ground.NO_HYPOTHESIS) and np.all(_twin(sweeps[-6])[0]["flags"] == ground.NO_HYPOTHESIS)
    with pytest.raises(api.StereoNetError, match="region of interest"):
        eng.ground(raw[:1], CAM, dataclasses.replace(BASE, roi_x=90, roi_y=40, roi_w=10, roi_h=10))      # leaves the image


@pytest.mark.gpu
def test_every_combination_of_outputs_and_every_call_form(eng):
    import torch
    raw = _maps()
    want = _twin()
    side = torch.cuda.Stream()
    for n, stream, combo in itertools.product((1, 3, MAX_BATCH), (0, side.cuda_stream), ((True, True), (True, False), (False, True))):
        assert not _differing(_device(torch, eng, raw[:n], CAM, BASE, want=combo, stream=stream), want, n), (n, stream, combo)
    for n in (1, 3, MAX_BATCH):                                                                           # host mode
        assert not _differing(eng.ground(raw[:n], CAM, BASE), want, n), n
        rec, lab = eng.ground(raw[:n], CAM, BASE, labels=False)
        assert lab is None and not _differing((rec, None), want, n)
    for k in range(MAX_BATCH):                                                                            # ten single calls
        assert not _differing(_device(torch, eng, raw[k:k + 1], CAM, BASE), (want[0][k:k + 1], want[1][k:k + 1])), k
    rec, lab = eng.ground(raw[4], CAM, BASE)                                                              # a 2-D map
    assert rec.tobytes() == want[0][4].tobytes() and np.array_equal(lab, want[1][4])
    pitch, roll = ground.angles(rec["base_from_cam"])
    assert abs(pitch - 0.2) < 2e-3 and abs(roll + 0.1) < 2e-3


@pytest.mark.gpu
def test_odd_shape_equals_twin(model_factory):
    """W % 4 == 2 and an odd height: no row starts 16-byte aligned, H * W is no multiple of 4 (the scalar label pass), the
    region's last sample row and column are partial tiles"""
    import torch
    w, h = 278, 75
    cam = Camera(fx=180.0, fy=175.0, cx=140.25, cy=30.5, baseline_mm=120.0)
    rng = np.random.default_rng(3)
    raw = np.stack([ground.scene(w, h, cam, 0.9, 0.15, 0.05, wall_z_m=9.0, boxes=2, hole_frac=0.05, outlier_frac=0.1, seed=8)[0],
                    rng.integers(-1000, 300000, (h, w)).astype(np.int32)])
    p = GroundParams(hypotheses=96, seed=3, refits=2, tol_px=0.05, min_inliers=500, min_area=50)
    with api.StereoNetHIP(model_factory(w, h, 64), max_batch=2) as e:
        for step in (1, 2, 4):
            c, q = dataclasses.replace(cam, step=step), dataclasses.replace(p, min_inliers=p.min_inliers // (step * step))
            want = ground.reference(raw, c, q, gate_q16=api.ground_gate(c, q, w, h))
            assert want[0]["flags"][0] & ground.FOUND and abs(want[0]["plane_cam"][0][3] - 0.9) < 5e-3, (step, want[0][0])
            assert not _differing(_device(torch, e, raw, c, q, shift=4 * (step > 1)), want), step
        assert not _differing(e.ground(raw, cam, p), ground.reference(raw, cam, p, gate_q16=api.ground_gate(cam, p, w, h)))      # host mode


@pytest.mark.gpu
def test_640x360_in_tiles_of_eight_rows_equals_twin(model_factory):
    """A call with 512 tiles or more takes tiles of eight sample rows, a smaller one (every other test here) tiles of fewer: four
    maps whose whole image is the region make 3 x 45 x 4 = 540, the last tile of every row of tiles partial; 64 hypotheses (four
    groups of lanes share a tile's rows) and 130 (every lane a hypothesis, and a second pass for two more)"""
    import torch
    w, h, n = 640, 360, 4
    cam = Camera(fx=400.0, fy=400.0, cx=320.5, cy=100.25, baseline_mm=120.0)
    raw = np.stack([ground.scene(w, h, cam, 0.5 + 0.2 * k, 0.1 * k, 0.04 * k - 0.05, wall_z_m=6.0 + k, boxes=2, hole_frac=0.05, outlier_frac=0.1, seed=20 + k)[0]
                    for k in range(n)])
    with api.StereoNetHIP(model_factory(w, h, 96), max_batch=n) as e:
        for K in (64, 130):
            p = GroundParams(roi_x=0, roi_y=0, roi_w=w, roi_h=h, hypotheses=K, seed=5, refits=1, tol_px=0.05, min_inliers=20000, min_area=500)
            want = ground.reference(raw, cam, p, gate_q16=api.ground_gate(cam, p, w, h))
            assert np.all(want[0]["flags"] & ground.FOUND) and np.abs(want[0]["plane_cam"][:, 3] - (0.5 + 0.2 * np.arange(n))).max() < 5e-3
            assert not _differing(_device(torch, e, raw, cam, p), want), K


@pytest.mark.gpu
def test_ground_beside_infer_batch(model_factory):
    """sn_infer_batch on one thread while another fits planes (ctypes drops the GIL): the records, the labels and the maps equal
    the serial run's."""
    raw = _maps()[:3]
    want = _twin()
    xs = np.stack([synth.model_input_i8(W, H, D, s) for s in range(3)])
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=3) as e:
        serial = e.infer(xs)[1]
        errors, rounds = [], []

        def work():
            try:
                for _ in range(12):
                    if _differing(e.ground(raw, CAM, BASE), want, 3):
                        errors.append("outputs differ")
                    rounds.append(1)
            except Exception as ex:        # noqa: BLE001
                errors.append(repr(ex))

        t = threading.Thread(target=work)
        t.start()
        try:
            for _ in range(5):
                assert np.array_equal(e.infer(xs)[1], serial)
        finally:
            t.join(60)
        assert not t.is_alive() and not errors and len(rounds) == 12, errors


OB = ObstacleParams(x_min_m=0.0, y_min_m=-2.0, cell_m=0.25, gw=28, gh=16, z_floor_m=-0.15, z_lo_m=0.1, z_hi_m=1.5, beams=31, angle_min_rad=-0.62,
                    angle_increment_rad=0.04, range_min_m=0.2, range_max_m=10.0)
OB_NAMES = ("occ", "hits", "height_mm", "ranges", "stats")


def _ob_sizes(n, p=OB):
    cells = p.gw * p.gh
    return (n * cells, n * cells * 8, n * cells * 4, n * p.beams * 4, n * 16)


def _ob_same(got, want):
    return [name for name, g, w_ in zip(OB_NAMES, got, want) if np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(w_).tobytes()]


@pytest.mark.gpu
def test_obstacles_with_ten_mounts_equal_ten_calls_and_the_twin(eng):
    import torch
    raw = _maps()
    mounts = np.float32([obstacles.mount(0.1 * k - 0.4, 0.03 * k, (0.05 * k, 0.0, 0.3 + 0.05 * k)) for k in range(MAX_BATCH)])
    edges = api.beam_edges(OB)
    singles = [eng.obstacles(raw[k], CAM, dataclasses.replace(OB, base_from_cam=tuple(float(v) for v in mounts[k]))) for k in range(MAX_BATCH)]
    singles = [np.stack([s[i] for s in singles]) for i in range(5)]
    twin = obstacles.reference(raw, CAM, dataclasses.replace(OB, base_from_cam=tuple(float(v) for v in mounts[0])), edges=edges)
    assert not _ob_same([s[:1] for s in singles], [t[:1] for t in twin]) and singles[4][:, :2].sum() > 1000
    # host mode; p->base_from_cam is ignored (here: not even finite)
    nan_ob = dataclasses.replace(OB, base_from_cam=(float("nan"),) * 12)
    assert not _ob_same(eng.obstacles(raw, CAM, nan_ob, mounts=mounts), singles)
    assert not _ob_same(eng.obstacles(raw[:3], CAM, OB, mounts=mounts[:3]), [s[:3] for s in singles])
    # device mode, the mounts inside records of 28 floats with guard words around every buffer
    recs = np.zeros(MAX_BATCH, ground.RECORD)
    recs["base_from_cam"] = mounts
    d_rec = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_raw = torch.from_numpy(raw.copy()).cuda()
    side = torch.cuda.Stream()
    for stream in (0, side.cuda_stream):
        bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") for s in _ob_sizes(MAX_BATCH)]
        torch.cuda.synchronize()
        eng.obstacles_device(MAX_BATCH, d_raw.data_ptr(), CAM, nan_ob, *[b.data_ptr() + GUARD for b in bufs], stream=stream,
                             mounts_ptr=d_rec.data_ptr() + 4 * ground.MOUNT_OFFSET_FLOATS, mount_stride=ground.RECORD_FLOATS)
        torch.cuda.synchronize()
        outs = [b.cpu().numpy() for b in bufs]
        assert all(np.all(o[:GUARD] == 0x5a) and np.all(o[-GUARD:] == 0x5a) for o in outs)
        assert not _ob_same([o[GUARD:-GUARD] for o in outs], singles), stream
    assert np.array_equal(d_rec.cpu().numpy(), recs.view(np.uint8))
    # argument errors of the new entry point
    lib, hnd, cam, prm = eng._lib, eng._h, eng._camera(CAM), api.obstacle_params(OB)
    ptr = [b.data_ptr() + GUARD for b in bufs]
    mp = d_rec.data_ptr() + 64
    for name, (m, stride) in {"null mounts": (0, 28), "misaligned mounts": (mp + 2, 28), "stride 11": (mp, 11), "mounts overlap occ": (ptr[0], 12)}.items():
        rc = lib.sn_obstacles_from_raw_mounts(hnd, 2, d_raw.data_ptr(), C.byref(cam), C.byref(prm), m or None, stride, *ptr, api.SN_MEM_DEVICE, None)
        assert rc == ERR_ARG and lib.sn_last_error(hnd).decode().startswith("sn_obstacles_from_raw_mounts: "), name


@pytest.mark.gpu
def test_chain_map_ground_obstacles_on_one_stream(eng):
    """sn_ground_from_raw -> sn_obstacles_from_raw_mounts on device buffers and one caller stream, nothing synchronised or brought
    to the host in between: the grid and the scan are the twin chain's, map by map"""
    import torch
    raw = _maps()
    d_raw = torch.from_numpy(raw.copy()).cuda()
    d_rec = torch.full((MAX_BATCH * REC,), 0x5a, dtype=torch.uint8, device="cuda")
    bufs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _ob_sizes(MAX_BATCH)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.ground_device(MAX_BATCH, d_raw.data_ptr(), CAM, BASE, d_rec.data_ptr(), 0, stream=st.cuda_stream)
    eng.obstacles_device(MAX_BATCH, d_raw.data_ptr(), CAM, OB, *[b.data_ptr() for b in bufs], stream=st.cuda_stream,
                         mounts_ptr=d_rec.data_ptr() + 4 * ground.MOUNT_OFFSET_FLOATS, mount_stride=ground.RECORD_FLOATS)
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy().view(ground.RECORD)
    assert not _differing((rec, None), _twin())
    edges = api.beam_edges(OB)
    twin = [obstacles.reference(raw[k], CAM, dataclasses.replace(OB, base_from_cam=tuple(float(v) for v in _twin()[0]["base_from_cam"][k])), edges=edges)
            for k in range(MAX_BATCH)]
    twin = [np.stack([t[i] for t in twin]) for i in range(5)]
    assert not _ob_same([b.cpu().numpy() for b in bufs], twin)
    assert twin[4][4, 1] > 500 and twin[4][3, 1] > 2000 and twin[4][3, 0] == 0      # the fitted mounts put the floors at z = 0: ground, not obstacle


@pytest.mark.gpu
def test_argument_errors_write_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    d_raw = torch.from_numpy(_maps().copy()).cuda()
    bufs = [torch.full((MAX_BATCH * REC,), 0x5a, dtype=torch.uint8, device="cuda"), torch.full((MAX_BATCH * H * W,), 0x5a, dtype=torch.uint8, device="cuda")]
    ok_cam = eng._camera(CAM)

    def call(n=1, r=None, c=ok_cam, prm=BASE, out=None, mem=api.SN_MEM_DEVICE, **kw):
        prm = api.ground_params(dataclasses.replace(prm, **kw)) if prm is not None else None
        out = [b.data_ptr() for b in bufs] if out is None else out
        r = d_raw.data_ptr() if r is None else r
        return lib.sn_ground_from_raw(hnd, n, r or None, C.byref(c) if c is not None else None, C.byref(prm) if prm is not None else None,
                                      *[o or None for o in out], mem, None)

    assert call() == 0 and call(n=MAX_BATCH) == 0                                  # the baseline calls are fine
    for b in bufs:
        b.fill_(0x5a)
    torch.cuda.synchronize()
    inf, nan = float("inf"), float("nan")
    ptr = [b.data_ptr() for b in bufs]
    bad = {"n = 0": dict(n=0), "n > max_batch": dict(n=MAX_BATCH + 1), "null raw": dict(r=0), "null camera": dict(c=None), "null params": dict(prm=None),
           "bad mem": dict(mem=7), "no outputs": dict(out=[0, 0]), "ground misaligned": dict(out=[ptr[0] + 4, ptr[1]]),
           "fx = 0": dict(c=api.SnCamera(0.0, 64.0, 48.0, 32.0, 120.0, 0.0, 0.0, 1)), "cx nan": dict(c=api.SnCamera(64.0, 64.0, nan, 32.0, 120.0, 0.0, 0.0, 1)),
           "cy inf": dict(c=api.SnCamera(64.0, 64.0, 48.0, inf, 120.0, 0.0, 0.0, 1)), "step 3": dict(c=api.SnCamera(64.0, 64.0, 48.0, 32.0, 120.0, 0.0, 0.0, 3)),
           "matrix nan": dict(base_from_cam=(nan,) + (0.0,) * 11), "hypotheses 0": dict(hypotheses=0), "hypotheses 1025": dict(hypotheses=1025),
           "refits 5": dict(refits=5), "refits negative": dict(refits=-1), "min_area negative": dict(min_area=-1), "min_inliers negative": dict(min_inliers=-1),
           "tol nan": dict(tol_px=nan), "tol negative": dict(tol_px=-0.1), "tol huge": dict(tol_px=9000.0), "tilt negative": dict(max_tilt_rad=-0.1),
           "tilt 1.6": dict(max_tilt_rad=1.6), "height_min 0": dict(height_min_m=0.0), "height_max < height_min": dict(height_max_m=0.1),
           "height_max inf": dict(height_max_m=inf), "region leaves the image": dict(roi_x=90, roi_y=40, roi_w=10, roi_h=10),
           "region below the image": dict(roi_x=0, roi_y=60, roi_w=10, roi_h=5), "region negative": dict(roi_x=-1, roi_y=40, roi_w=10, roi_h=10),
           "region without width": dict(roi_x=0, roi_y=40, roi_w=0, roi_h=10), "two samples": dict(roi_x=0, roi_y=40, roi_w=2, roi_h=1),
           "raw overlaps ground": dict(out=[d_raw.data_ptr() + 4 * H * W - 8, ptr[1]]), "ground overlaps labels": dict(out=[ptr[0], ptr[0] + 8])}
    for name, kw in bad.items():
        rc = call(**kw)
        msg = lib.sn_last_error(hnd).decode()
        assert rc == ERR_ARG and msg.startswith("sn_ground_from_raw: ") and len(msg) > len("sn_ground_from_raw: "), (name, rc, msg)
    rc = call(c=api.SnCamera(64.0, 64.0, 48.0, 32.0, 120.0, 0.0, 0.0, 4), roi_x=1, roi_y=41, roi_w=3, roi_h=3)      # between the step's grid lines
    assert rc == ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((b == 0x5a).all()) for b in bufs)
    assert lib.sn_ground_from_raw(None, 1, d_raw.data_ptr(), C.byref(ok_cam), C.byref(api.ground_params(BASE)), *ptr, api.SN_MEM_DEVICE, None) == ERR_ARG
    gate = np.zeros(6, np.int64)
    assert lib.sn_ground_gate(C.byref(ok_cam), C.byref(api.ground_params(BASE)), 9000, H, gate.ctypes.data) == ERR_ARG and not gate.any()


@pytest.mark.gpu
def test_destroy_after_use_leaves_nothing_behind(model_factory):
    """Engines that used the stage in every form are created and closed in turn: the device's free memory does not go down from
    one turn to the next (one turn's staging is some 6 MB at this size; the slack is about that)."""
    import torch
    w, h, n = 640, 360, 4
    rng = np.random.default_rng(1)
    raw = rng.integers(1, 1 << 18, (n, h, w), dtype=np.int64).astype(np.int32)
    cam = Camera(fx=400.0, fy=400.0, baseline_mm=120.0)
    p = GroundParams(hypotheses=1024, refits=4)
    model = model_factory(w, h, 96)

    def turn():
        with api.StereoNetHIP(model, max_batch=n) as e:
            e.ground(raw, cam, p)
            d_raw = torch.from_numpy(raw).cuda()
            d_lab = torch.empty(n * h * w, dtype=torch.uint8, device="cuda")      # labels without records: the lane's own
            e.ground_device(n, d_raw.data_ptr(), cam, p, 0, d_lab.data_ptr())
            del d_raw, d_lab
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0]

    turn()
    free = [turn() for _ in range(4)]
    assert min(free[1:]) >= free[0] - (8 << 20), free


def _found_params(raw, cam, **kw):
    """parameters under which the twin finds a plane in `raw`, whatever the engine made of its synthetic weights: a gate as wide
    as it goes, and the narrowest of a few inlier bands that gives a plane holding a tenth of the region"""
    for tol in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        p = GroundParams(hypotheses=512, seed=2, refits=2, tol_px=tol, min_inliers=W * (H // 2) // 10, min_area=16, max_tilt_rad=1.5, height_min_m=0.01,
                         height_max_m=100.0, **kw)
        if ground.reference(raw, cam, p, labels=False)[0]["flags"] & ground.FOUND:
            return p
    raise AssertionError("no plane in the engine's map")


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    r = subprocess.run([os.path.join(COMPAT, "build", "obstacle_harness"), model, frames, str(W), str(H), str(nframes), prefix],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    msgs = [open(f"{prefix}.{i}.msg", "rb").read() for i in range(nframes)]
    grids = [open(f"{prefix}.{i}.grid", "rb").read() for i in range(nframes) if os.path.exists(f"{prefix}.{i}.grid")]
    return msgs, grids, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_gives_the_obstacle_stage_every_frames_mount(weights_blob, tmp_path):
    """STEREONET_GROUND beside STEREONET_OBSTACLES: the grid on /stereonet_obstacle_grid is the twin chain's (the plane of the
    frame's map, its mount, the grid under that mount), not the grid of the obstacle file's own mount"""
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 2
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(str(tmp_path / "f.bin"))
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    with api.StereoNetHIP(m) as e:
        first = e.infer_sbs_nv12(sbs)[1].reshape(H, W)
    gp = _found_params(first, cam, base_from_cam=obstacles.mount(0.0, 0.0, (0.0, 0.0, 0.3)), log_delta=0.001)
    ob = ObstacleParams(x_min_m=0.0, y_min_m=-3.0, cell_m=0.15, gw=40, gh=40, z_floor_m=-0.5, z_lo_m=0.05, z_hi_m=2.0, min_obstacle_hits=1, min_ground_hits=1)
    ground.save_params(str(tmp_path / "ground.txt"), gp)
    obstacles.save_params(str(tmp_path / "ob.txt"), ob)
    env = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_OBSTACLES": str(tmp_path / "ob.txt")}
    plain, grids0, _ = _run_harness(tmp_path, "file", m, str(tmp_path / "f.bin"), nframes, env)
    msgs, grids, log = _run_harness(tmp_path, "fit", m, str(tmp_path / "f.bin"), nframes, dict(env, STEREONET_GROUND=str(tmp_path / "ground.txt")))
    assert msgs == plain and len(grids) == len(grids0) == nframes and "ground: found, height" in log
    gate = api.ground_gate(cam, gp, W, H)
    for k in range(nframes):
        raw = np.frombuffer(msgs[k][:4 * W * H], np.int32).reshape(H, W)
        rec, _ = ground.reference(raw, cam, gp, gate_q16=gate, labels=False)
        assert rec["flags"] & ground.FOUND
        occ = obstacles.reference(raw, cam, dataclasses.replace(ob, base_from_cam=tuple(float(v) for v in rec["base_from_cam"])))[0]
        assert grids[k] == occ.tobytes() and grids0[k] == obstacles.reference(raw, cam, ob)[0].tobytes(), k
        assert grids[k] != grids0[k] and (occ != -1).any()
    # a file the stage refuses leaves the obstacle stage with its own mount
    ground.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(gp, hypotheses=0))
    msgs, grids, log = _run_harness(tmp_path, "bad", m, str(tmp_path / "f.bin"), nframes, dict(env, STEREONET_GROUND=str(tmp_path / "bad.txt")))
    assert msgs == plain and grids == grids0 and log.count("no ground plane") == 1


@pytest.mark.gpu
def test_filelist_writes_the_record_and_the_labels(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    rng = np.random.default_rng(11)
    lists = {}
    for eye in ("left", "right"):
        paths = []
        for i in range(2):
            path = str(tmp_path / f"{eye}{i}.ppm")
            images.write_ppm(path, rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            paths.append(path)
        lists[eye] = str(tmp_path / f"{eye}.list")
        with open(lists[eye], "w") as f:
            f.write("\n".join(paths) + "\n")
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    with api.StereoNetHIP(model_factory(W, H, D)) as e:
        eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}0.ppm"))) for eye in ("left", "right")]
        gp = _found_params(e.infer_sbs_nv12(images.sbs_from_eyes(eyes[0], eyes[1], W, H))[1].reshape(H, W), cam)
    ob = ObstacleParams(x_min_m=0.0, y_min_m=-3.0, cell_m=0.15, gw=40, gh=40, z_floor_m=-0.5, z_lo_m=0.05, z_hi_m=2.0, min_obstacle_hits=1, min_ground_hits=1)
    ground.save_params(str(tmp_path / "ground.txt"), gp)
    obstacles.save_params(str(tmp_path / "ob.txt"), ob)
    out = str(tmp_path / "out")
    common = ["--model", model_factory(W, H, D), "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120"]
    assert filelist.main(common + ["--out", out, "--ground", str(tmp_path / "ground.txt"), "--obstacles", str(tmp_path / "ob.txt")]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    gate = api.ground_gate(cam, gp, W, H)
    for i in range(2):
        raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)      # the final map of the chain
        rec, lab = ground.reference(raw, cam, gp, gate_q16=gate)
        ground.write_record(str(tmp_path / "want.txt"), rec)
        assert open(os.path.join(out, f"{i}.ground.txt")).read() == open(tmp_path / "want.txt").read()
        assert open(os.path.join(out, f"{i}.ground.pgm"), "rb").read() == b"P5\n%d %d\n255\n" % (W, H) + ground.labels_image(lab).tobytes()
        occ = obstacles.reference(raw, cam, dataclasses.replace(ob, base_from_cam=tuple(float(v) for v in rec["base_from_cam"])))[0]
        assert open(os.path.join(out, f"{i}.grid.pgm"), "rb").read() == b"P5\n40 40\n255\n" + obstacles.grid_image(occ).tobytes()
        pitch, roll = ground.angles(rec["base_from_cam"])
        assert summary["ground_found"][i] == bool(rec["flags"] & ground.FOUND) and summary["inliers"][i] == int(rec["inliers"])
        assert summary["height_m"][i] == float(rec["plane_cam"][3]) and summary["pitch_deg"][i] == math.degrees(pitch) and summary["roll_deg"][i] == math.degrees(roll)
    assert summary["ground_found"][0] is True
    with pytest.raises(SystemExit):
        filelist.main(common + ["--ground", str(tmp_path / "ground.txt")])      # needs --out
