"""sn_obstacles_from_raw on the MI355X: the grid, the counts, the heights, the scan and the statistics equal the numpy twin's
(hobot_stereonet_amd/obstacles.py) byte for byte on constructed maps that put points exactly on every boundary of the contract,
for every step, every combination of outputs, every call form, with guard bytes untouched; 1242x375 (W % 4 == 2, an odd
height); the run-length and the plain accumulation; a batch against single calls; beside inference; end to end from the
engine's own map on the device; argument errors; what sn_destroy leaves behind; the node's two topics and the filelist tool.

No tolerance appears: the contract is the same bytes.  The twin is fed the library's beam table (the two tables may differ by an
ulp, tests/test_obstacles.py)."""
import ctypes as C
import dataclasses
import functools
import itertools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from hobot_stereonet_amd import api, obstacles, synth, weights
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG = -1                    # SN_ERR_ARG (include/stereonet_hip.h)
NAMES = ("occ", "hits", "height_mm", "ranges", "stats")
f32 = np.float32
CAM = Camera(fx=64.0, fy=64.0, cx=48.0, cy=32.0, baseline_mm=120.0)
PLANE_RAW = 9000                # the fronto-parallel plane of map 0: Z = 1.71 m


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


@functools.lru_cache(maxsize=None)
def _maps():
    """ten different maps, shared by the tests and never changed: 0 a fronto-parallel plane (a constant: the contention case), 1
    zeros, 2 a ground plane and a wall, 3 and 4 random words whose neighbouring rows disagree (depths of 0.5 .. 8 m, zeros and
    negative words among them), 5 any int32 word, 6 a ramp, 7 the plane with holes, 8 a nearer plane, 9 the wall scene again,
    farther"""
    rng = np.random.default_rng(5)
    raw = np.zeros((MAX_BATCH, H, W), np.int32)
    raw[0] = PLANE_RAW
    raw[2] = obstacles.ground_and_wall(W, H, CAM, 0.5, 3.1)
    for k in (3, 4):
        raw[k] = rng.integers(2400, 38400, (H, W))
        raw[k][rng.random((H, W)) < 0.1] = 0
        raw[k][rng.random((H, W)) < 0.05] = -rng.integers(1, 1 << 30)
    raw[5] = rng.integers(-(1 << 31), 1 << 31, (H, W), dtype=np.int64).astype(np.int32)
    raw[6] = np.linspace(1000, 60000, H * W).reshape(H, W).astype(np.int32)
    raw[7] = PLANE_RAW
    raw[7][::3, ::5] = 0
    raw[8] = 30000
    raw[9] = obstacles.ground_and_wall(W, H, CAM, 0.4, 5.7)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (camera, parameters).  `edges` puts the plane of map 0 exactly on every boundary: its x on a cell edge (x_min_m is
    the plane's xb minus three cells, exact in fp32), the column u = cx at yb = 0 on a cell edge and at t = 0 on the beam edge
    tan(0), the row v = cy at zb = t_z = z_lo_m, two other rows' zb as z_floor_m and z_hi_m, two pixels' ranges as range_min_m
    and range_max_m, the plane's depth as the camera's z_max_m (map 8 is nearer than its z_min_m, the random maps lie on
    either side of both); its grid is smaller than the view on all four sides."""
    level = obstacles.mount(t=(0.0, 0.0, 0.5))
    probe = ObstacleParams(base_from_cam=level)
    xb, yb, zb = (a[0] for a in obstacles.base_points(_maps()[0], CAM, probe))
    z_plane = float(xb[0, 0])
    assert np.all(xb == xb[0, 0]) and yb[0, 48] == 0 and zb[32, 0] == f32(0.5)
    r = np.sqrt(xb * xb + yb * yb)
    edges_cam = dataclasses.replace(CAM, z_min_m=0.9, z_max_m=z_plane)
    cases = {
        "edges": (edges_cam, ObstacleParams(base_from_cam=level, x_min_m=float(f32(z_plane) - f32(0.75)), y_min_m=-1.0, cell_m=0.25, gw=5, gh=8,
                                            z_floor_m=float(zb[50, 0]), z_lo_m=0.5, z_hi_m=float(zb[10, 0]), min_obstacle_hits=2, min_ground_hits=2,
                                            beams=8, angle_min_rad=-0.5, angle_increment_rad=0.125, range_min_m=float(r[20, 44]),
                                            range_max_m=float(r[20, 70]))),
        "wall": (CAM, ObstacleParams(base_from_cam=level, x_min_m=0.0, y_min_m=-2.0, cell_m=0.25, gw=28, gh=16, z_floor_m=-0.15, z_lo_m=0.1,
                                     z_hi_m=1.5, beams=31, angle_min_rad=-0.62, angle_increment_rad=0.04, range_min_m=0.2, range_max_m=10.0)),
        # a mount yawed by 120 degrees and pitched: most points have xb <= 0
        "yawed": (CAM, ObstacleParams(base_from_cam=obstacles.mount(2.0943951, 0.15, (0.2, -0.1, 0.7)), x_min_m=-3.0, y_min_m=-1.0,
                                      cell_m=0.3, gw=17, gh=23, z_floor_m=-0.4, z_lo_m=0.2, z_hi_m=2.5, min_obstacle_hits=1, min_ground_hits=4,
                                      beams=100, angle_min_rad=-1.5, angle_increment_rad=0.03, range_min_m=0.5, range_max_m=6.0)),
        # every pixel of a map in one cell and one beam
        "one cell": (CAM, ObstacleParams(x_min_m=-32.0, y_min_m=-32.0, cell_m=64.0, gw=1, gh=1, z_floor_m=-50.0, z_lo_m=-40.0, z_hi_m=50.0,
                                         beams=1, angle_min_rad=-1.2, angle_increment_rad=2.4, range_min_m=0.0, range_max_m=1000.0)),
        "grid only": (CAM, ObstacleParams(base_from_cam=level, x_min_m=0.5, y_min_m=-1.5, cell_m=0.125, gw=40, gh=24, beams=0)),
        "scan only": (CAM, ObstacleParams(base_from_cam=level, gw=0, gh=0, z_floor_m=-0.15, z_lo_m=0.1, z_hi_m=1.5, beams=4096,
                                          angle_min_rad=-0.7, angle_increment_rad=1.4 / 4096, range_min_m=0.0, range_max_m=20.0)),
    }
    p = cases["edges"][1]
    assert p.x_min_m + 0.75 == z_plane and p.z_floor_m < 0.5 < p.z_hi_m and p.range_min_m < p.range_max_m
    return cases


@functools.lru_cache(maxsize=None)
def _twin(name, step=1):
    """the twin on the ten maps with the library's beam table: (occ, hits, height_mm, ranges, stats), read-only"""
    cam, p = _cases()[name]
    out = obstacles.reference(_maps(), dataclasses.replace(cam, step=step), p, edges=api.beam_edges(p) if p.beams else None)
    for a in out:
        a.setflags(write=False)
    return out


def _fit(raw, cam, frame="base_link"):
    """parameters under which the valid points of `raw` fill a 40 x 36 grid and a 64-beam scan, whatever its depths are: the
    bounds are percentiles of the twin's own base-frame coordinates, rounded to fp32"""
    level = obstacles.mount(t=(0.0, 0.0, 0.3))
    xb, yb, zb = obstacles.base_points(raw, cam, ObstacleParams(base_from_cam=level))
    ok = np.isfinite(xb)
    assert ok.sum() > 500, "the engine's map holds too few measurements"
    q = lambda a, pc: float(f32(np.percentile(a[ok].astype(np.float64), pc)))      # noqa: E731
    x0, x1, y0, y1 = q(xb, 5), q(xb, 95), q(yb, 5), q(yb, 95)
    cell = float(f32(max((x1 - x0) / 40, (y1 - y0) / 36, 1e-3)))
    return ObstacleParams(base_from_cam=level, x_min_m=x0, y_min_m=y0, cell_m=cell, gw=40, gh=36, z_floor_m=q(zb, 5), z_lo_m=q(zb, 50),
                          z_hi_m=q(zb, 95), min_obstacle_hits=1, min_ground_hits=1, beams=64, angle_min_rad=-0.64, angle_increment_rad=0.02,
                          range_min_m=0.0, range_max_m=float(f32(2 * x1 + 1)), frame=frame)


def _sizes(n, p):
    cells = p.gw * p.gh
    return (n * cells, n * cells * 8, n * cells * 4, n * p.beams * 4, n * 16)


def _shaped(n, p, parts):
    dt = (np.int8, np.uint32, np.int32, np.float32, np.uint32)
    shapes = ((n, p.gh, p.gw), (n, p.gh, p.gw, 2), (n, p.gh, p.gw), (n, p.beams), (n, 4))
    return [None if b is None else b.view(d).reshape(s) for b, d, s in zip(parts, dt, shapes)]


def _all(p):
    """every output the parameters allow"""
    return (p.gw > 0, p.gw > 0, p.gw > 0, p.beams > 0, p.gw > 0)


def _device(torch, e, raw, cam, p, want=None, stream=0, shift=0):
    """device mode: every wanted output (default: all the parameters allow) GUARD bytes into a buffer of 0x5a of its own, raw
    `shift` bytes into its buffer -> the five outputs (None where not wanted), after checking every byte the call must not write"""
    n = raw.shape[0]
    want = _all(p) if want is None else want
    d_raw = torch.zeros(raw.size * 4 + shift + 16, dtype=torch.uint8, device="cuda")
    d_raw[shift:shift + raw.size * 4].copy_(torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1).copy()))
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(_sizes(n, p), want)]
    torch.cuda.synchronize()
    e.obstacles_device(n, d_raw.data_ptr() + shift, cam, p, *[b.data_ptr() + GUARD if b is not None else 0 for b in bufs], stream=stream)
    if stream:
        torch.cuda.synchronize()
    parts = []
    for name, b, s in zip(NAMES, bufs, _sizes(n, p)):
        if b is None:
            parts.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a), f"guard bytes around {name}"
        parts.append(o[GUARD:GUARD + s].copy())
    return _shaped(n, p, parts)


def _differing(got, want, n=None):
    """the names of the outputs whose bytes differ from the twin's first n maps"""
    bad = []
    for name, g, w_ in zip(NAMES, got, want):
        if g is None:
            continue
        w_ = w_ if n is None else w_[:n]
        if g.shape != w_.shape or g.tobytes() != np.ascontiguousarray(w_).tobytes():
            bad.append(name)
    return bad


@pytest.mark.gpu
def test_bytes_equal_twin_on_every_boundary_and_step(eng):
    import torch
    raw = _maps()
    bad, calls = [], 0
    for name, (cam, p) in _cases().items():
        for step in (1, 2, 4):
            want = _twin(name, step)
            for shift in (0, 4):                        # a map base that is 4- but not 16-byte aligned
                got = _device(torch, eng, raw, dataclasses.replace(cam, step=step), p, shift=shift)
                calls += 1
                if _differing(got, want):
                    bad.append((name, step, shift, _differing(got, want)))
    print(f"{calls} device calls of n = {MAX_BATCH}, {len(bad)} differ")
    assert not bad, bad
    # the inputs do what they were built for
    occ, hits, height, ranges, stats = _twin("edges")
    assert hits[0, :, 3].sum() > 0 and hits[0, :, 2].sum() == 0            # the plane sits on the edge of column 3, not in 2
    assert hits[0].sum() < H * W and hits[8].sum() == 0 and hits[1].sum() == 0 and 0 < hits[3].sum() < hits[0].sum()
    assert np.isfinite(ranges[0]).any() and np.isinf(ranges[0]).any()
    assert np.array_equal(hits.sum(axis=(1, 2)), stats[:, :2])             # summed hits equal stats
    occ, hits, height, ranges, stats = _twin("one cell")
    assert int(hits[0].sum()) == H * W and np.isfinite(ranges[0, 0]) and stats[0, 2] == 1
    occ, hits, height, ranges, stats = _twin("yawed")
    assert hits.sum() > 0 and np.isfinite(ranges).any()
    occ, hits, height, ranges, stats = _twin("wall")
    assert set(np.unique(occ[2]).tolist()) == {-1, 0, 100} and np.isfinite(ranges[2]).sum() > 20


@pytest.mark.gpu
def test_every_combination_of_outputs(eng):
    import torch
    raw = _maps()[:3]
    cam, p = _cases()["wall"]
    want = _twin("wall")
    lib, hnd = eng._lib, eng._h
    for combo in itertools.product((0, 1), repeat=5):
        if any(combo[:4]):
            got = _device(torch, eng, raw, cam, p, want=combo)
            assert [g is not None for g in got] == [bool(c) for c in combo] and not _differing(got, want, 3), combo
        else:                                          # stats alone, or nothing at all
            d_raw = torch.from_numpy(raw.copy()).cuda()
            d_st = torch.full((64,), 0x5a, dtype=torch.uint8, device="cuda")
            c, prm = eng._camera(cam), api.obstacle_params(p)
            rc = lib.sn_obstacles_from_raw(hnd, 3, d_raw.data_ptr(), C.byref(c), C.byref(prm), None, None, None, None,
                                           d_st.data_ptr() if combo[4] else None, api.SN_MEM_DEVICE, None)
            torch.cuda.synchronize()
            assert rc == ERR_ARG and bool((d_st == 0x5a).all()), combo
    # a grid without a scan and a scan without a grid: what the other half would need is refused
    for name, refused in (("grid only", 3), ("scan only", 0)):
        cam, p = _cases()[name]
        flags = list(_all(p))
        assert not _differing(_device(torch, eng, raw, cam, p, want=flags), _twin(name), 3), name
        flags[refused] = True
        with pytest.raises(api.StereoNetError):
            _device(torch, eng, raw, cam, p, want=flags)


@pytest.mark.gpu
def test_every_call_form_and_a_batch_against_single_calls(eng):
    import torch
    raw = _maps()
    side = torch.cuda.Stream()
    for name in ("edges", "yawed", "one cell"):
        cam, p = _cases()[name]
        want = _twin(name)
        for n in (1, MAX_BATCH):
            assert not _differing(eng.obstacles(raw[:n], cam, p), want, n), (name, n)                      # host mode
            for stream in (0, side.cuda_stream):                                                          # blocking | a caller stream
                assert not _differing(_device(torch, eng, raw[:n], cam, p, stream=stream), want, n), (name, n, stream)
        for k in range(MAX_BATCH):                                                                        # ten single calls
            got = _device(torch, eng, raw[k:k + 1], cam, p)
            assert not _differing(got, [w_[k:k + 1] for w_ in want]), (name, k)
        single = eng.obstacles(raw[2], cam, p)                                                            # a 2-D map
        assert all(np.array_equal(a, b[2], equal_nan=True) for a, b in zip(single, want))
    # without a grid or a scan the host form hands back empty arrays
    cam, p = _cases()["wall"]
    occ, hits, height, ranges, stats = eng.obstacles(raw[:2], cam, p, grid=False)
    assert occ.size == 0 and np.array_equal(ranges.view(np.uint32), _twin("wall")[3][:2].view(np.uint32))
    occ, hits, height, ranges, stats = eng.obstacles(raw[:2], cam, p, scan=False)
    assert ranges.size == 0 and np.array_equal(occ, _twin("wall")[0][:2]) and np.array_equal(stats, _twin("wall")[4][:2])


@pytest.mark.gpu
def test_run_length_and_plain_accumulation_give_the_same_bytes(model_factory, monkeypatch):
    """SN_OBSTACLE_RLE=0 (read by sn_create): one set of atomics per point instead of one per run of a lane"""
    import torch
    raw = _maps()
    monkeypatch.setenv("SN_OBSTACLE_RLE", "0")
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as plain:
        monkeypatch.delenv("SN_OBSTACLE_RLE")
        with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as rle:
            for name, (cam, p) in _cases().items():
                for step in (1, 2):
                    c = dataclasses.replace(cam, step=step)
                    a, b = _device(torch, plain, raw, c, p), _device(torch, rle, raw, c, p)
                    assert not _differing(a, b) and not _differing(a, _twin(name, step)), (name, step)


@pytest.mark.gpu
def test_1242x375_equals_twin(model_factory):
    import torch
    w, h = 1242, 375                                    # W % 4 == 2 and an odd height; five column blocks, the last one partial
    cam = Camera(fx=700.0, fy=700.0, cx=620.5, cy=180.25, baseline_mm=120.0)
    rng = np.random.default_rng(3)
    raw = np.stack([obstacles.ground_and_wall(w, h, cam, 1.2, 14.0),
                    rng.integers(-1000, 300000, (h, w)).astype(np.int32)])
    p = ObstacleParams(base_from_cam=obstacles.mount(0.05, 0.02, (0.3, 0.0, 1.2)), x_min_m=0.0, y_min_m=-8.0, cell_m=0.2, gw=100, gh=80,
                       z_floor_m=-0.2, z_lo_m=0.15, z_hi_m=2.0, beams=360, angle_min_rad=-0.9, angle_increment_rad=0.005, range_min_m=0.3,
                       range_max_m=30.0)
    with api.StereoNetHIP(model_factory(w, h, 256), max_batch=2) as e:
        edges = api.beam_edges(p)
        for step in (1, 2, 4):
            c = dataclasses.replace(cam, step=step)
            want = obstacles.reference(raw, c, p, edges=edges)
            assert want[4][0, 2] > 0 and want[4][0, 3] > 0 and np.isfinite(want[3]).any()
            assert not _differing(_device(torch, e, raw, c, p, shift=4 * (step > 1)), want), step
        assert not _differing(e.obstacles(raw, cam, p), obstacles.reference(raw, cam, p, edges=edges))      # host mode


@pytest.mark.gpu
def test_obstacles_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread reduces maps (ctypes drops the GIL): the outputs and the maps equal the
    serial run's."""
    raw = _maps()[:3]
    cam, p = _cases()["wall"]
    want = _twin("wall")
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=3) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, rounds = [], []

        def work():
            try:
                for _ in range(12):
                    if _differing(e.obstacles(raw, cam, p), want, 3):
                        errors.append("outputs differ")
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
def test_end_to_end_on_the_device_from_the_engines_own_map(eng):
    """sn_infer_batch -> sn_obstacles_from_raw on one stream, nothing crosses to the host in between"""
    import torch
    n = 3
    x = np.stack([synth.model_input_i8(W, H, D, 20 + k) for k in range(n)])
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    p = _fit(np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)]), cam)      # fitted to the maps the chain will make
    d_in = torch.from_numpy(x).cuda()
    d_raw = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    sizes = _sizes(n, p)
    bufs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.infer_device(n, d_in.data_ptr(), d_raw.data_ptr(), 0, stream=st.cuda_stream)
    eng.obstacles_device(n, d_raw.data_ptr(), cam, p, *[b.data_ptr() for b in bufs], stream=st.cuda_stream)
    torch.cuda.synchronize()
    raw = d_raw.cpu().numpy()
    want = obstacles.reference(raw, cam, p, edges=api.beam_edges(p), out_scale=eng.out_scale)
    assert np.array_equal(raw, np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)]))
    assert want[4][:, :2].sum() > 1000 and (want[4][:, 2:] > 0).all() and np.isfinite(want[3]).any()      # a scene, not an empty grid
    assert not _differing(_shaped(n, p, [b.cpu().numpy() for b in bufs]), want)


@pytest.mark.gpu
def test_argument_errors_write_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    raw = _maps()
    cam, p = _cases()["wall"]
    sizes = _sizes(MAX_BATCH, p)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    bufs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    ok_cam = eng._camera(cam)

    def call(n=1, r=None, c=ok_cam, prm=p, out=None, mem=api.SN_MEM_DEVICE, **kw):
        prm = api.obstacle_params(dataclasses.replace(prm, **kw)) if prm is not None else None
        out = [b.data_ptr() for b in bufs] if out is None else out
        r = d_raw.data_ptr() if r is None else r
        return lib.sn_obstacles_from_raw(hnd, n, r or None, C.byref(c) if c is not None else None, C.byref(prm) if prm is not None else None,
                                         *[o or None for o in out], mem, None)

    assert call() == 0 and call(n=MAX_BATCH) == 0                                  # the baseline calls are fine
    for b in bufs:
        b.fill_(0x5a)
    torch.cuda.synchronize()
    inf, nan = float("inf"), float("nan")
    ptr = [b.data_ptr() for b in bufs]
    bad = {"n = 0": dict(n=0), "n > max_batch": dict(n=MAX_BATCH + 1), "null raw": dict(r=0), "null camera": dict(c=None),
           "null params": dict(prm=None), "bad mem": dict(mem=7), "no outputs": dict(out=[0, 0, 0, 0, 0]), "stats alone": dict(out=[0, 0, 0, 0, ptr[4]]),
           "fx = 0": dict(c=api.SnCamera(0.0, 64.0, 48.0, 32.0, 120.0, 0.0, 0.0, 1)), "fy nan": dict(c=api.SnCamera(64.0, nan, 48.0, 32.0, 120.0, 0.0, 0.0, 1)),
           "baseline 0": dict(c=api.SnCamera(64.0, 64.0, 48.0, 32.0, 0.0, 0.0, 0.0, 1)), "step 3": dict(c=api.SnCamera(64.0, 64.0, 48.0, 32.0, 120.0, 0.0, 0.0, 3)),
           "matrix nan": dict(base_from_cam=(nan,) + (0.0,) * 11), "matrix inf": dict(base_from_cam=(0.0,) * 11 + (inf,)),
           "x_min nan": dict(x_min_m=nan), "y_min inf": dict(y_min_m=inf), "cell nan": dict(cell_m=nan), "cell 0": dict(cell_m=0.0),
           "cell negative": dict(cell_m=-0.25), "gw > 4096": dict(gw=4097), "gh > 4096": dict(gh=4097), "gw negative": dict(gw=-1),
           "gw 0 with gh": dict(gw=0), "beams > 4096": dict(beams=4097), "beams negative": dict(beams=-1), "z_floor nan": dict(z_floor_m=nan),
           "z_floor > z_lo": dict(z_floor_m=0.2), "z_lo > z_hi": dict(z_lo_m=1.6), "z_hi inf": dict(z_hi_m=inf),
           "obstacle hits negative": dict(min_obstacle_hits=-1), "ground hits negative": dict(min_ground_hits=-1),
           "range_min negative": dict(range_min_m=-0.1), "range_max < range_min": dict(range_max_m=0.1), "range_max inf": dict(range_max_m=inf),
           "angle nan": dict(angle_min_rad=nan), "sector beyond pi/2": dict(angle_increment_rad=0.08), "increment 0": dict(angle_increment_rad=0.0),
           "no grid but grid outputs": dict(gw=0, gh=0), "no scan but ranges": dict(beams=0),
           "raw overlaps hits": dict(out=[ptr[0], d_raw.data_ptr() + 4 * H * W - 4, ptr[2], ptr[3], ptr[4]]),
           "occ overlaps height": dict(out=[ptr[2] + 8, ptr[1], ptr[2], ptr[3], ptr[4]]),
           "ranges overlaps stats": dict(out=[ptr[0], ptr[1], ptr[2], ptr[3], ptr[3] + 4])}
    for name, kw in bad.items():
        rc = call(**kw)
        msg = lib.sn_last_error(hnd).decode()
        assert rc == ERR_ARG and msg.startswith("sn_obstacles_from_raw: ") and len(msg) > len("sn_obstacles_from_raw: "), (name, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5a).all()) for b in bufs)
    assert lib.sn_obstacles_from_raw(None, 1, d_raw.data_ptr(), C.byref(ok_cam), C.byref(api.obstacle_params(p)), *ptr, api.SN_MEM_DEVICE, None) == ERR_ARG
    with pytest.raises(api.StereoNetError):
        eng.obstacles(raw[:1], cam, dataclasses.replace(p, cell_m=0.0))


@pytest.mark.gpu
def test_destroy_after_use_leaves_nothing_behind(model_factory):
    """Engines that used the stage in every form are created and closed in turn: the device's free memory does not go down from
    one turn to the next (one turn's staging is some 7 MB at this size; the slack is about that)."""
    import torch
    w, h, n = 640, 360, 4
    rng = np.random.default_rng(1)
    raw = rng.integers(1, 1 << 18, (n, h, w), dtype=np.int64).astype(np.int32)
    cam = Camera(fx=400.0, fy=400.0, baseline_mm=120.0)
    p = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), cell_m=0.05, gw=400, gh=400, beams=720, angle_min_rad=-0.72,
                       angle_increment_rad=0.002, range_max_m=30.0)
    model = model_factory(w, h, 96)

    def turn():
        with api.StereoNetHIP(model, max_batch=n) as e:
            e.obstacles(raw, cam, p)
            d_raw = torch.from_numpy(raw).cuda()
            d_occ = torch.empty(n * p.gw * p.gh, dtype=torch.int8, device="cuda")      # occ without hits: the lane's own counts
            e.obstacles_device(n, d_raw.data_ptr(), cam, p, occ_ptr=d_occ.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        del d_raw, d_occ
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    turn()                                  # the runtime's own pools exist after the first
    free = [turn() for _ in range(3)]
    print("free bytes after each turn:", free)
    assert free[2] >= free[0] - (8 << 20), free


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    r = subprocess.run([os.path.join(COMPAT, "build", "obstacle_harness"), model, frames, str(W), str(H), str(nframes), prefix],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    msgs = [open(f"{prefix}.{i}.msg", "rb").read() for i in range(nframes)]
    lines = r.stdout.splitlines()
    grids = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("grid ")]
    scans = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("scan ")]
    return msgs, grids, scans, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_grid_and_the_scan(weights_blob, tmp_path):
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 3
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(str(tmp_path / "f.bin"))
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0, z_min_m=0.05)
    with api.StereoNetHIP(m) as e:
        p = _fit(e.infer_sbs_nv12(sbs)[1].reshape(H, W), cam, frame="base_footprint")
    obstacles.save_params(str(tmp_path / "ob.txt"), p)
    cam_env = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0"}
    plain, g0, s0, _ = _run_harness(tmp_path, "plain", m, str(tmp_path / "f.bin"), nframes, {})
    assert not g0 and not s0                                              # unset: nothing on either topic
    msgs, grids, scans, log = _run_harness(tmp_path, "on", m, str(tmp_path / "f.bin"), nframes,
                                           dict(cam_env, STEREONET_OBSTACLES=str(tmp_path / "ob.txt")))
    assert msgs == plain and len(grids) == len(scans) == nframes and "/stereonet_obstacle_grid" in log
    edges = api.beam_edges(p)
    for k in range(nframes):
        raw = np.frombuffer(msgs[k][:4 * W * H], np.int32).reshape(H, W)
        occ, _, _, ranges, _ = obstacles.reference(raw, cam, p, edges=edges)
        assert open(tmp_path / f"on.{k}.grid", "rb").read() == occ.tobytes() and (occ == 100).any(), k
        assert open(tmp_path / f"on.{k}.scan", "rb").read() == ranges.tobytes() and np.isfinite(ranges).any(), k
        g, s = grids[k], scans[k]
        assert g["frame_id"] == s["frame_id"] == "base_footprint" and g["stamp"] == s["stamp"] == f"7.{1000 + k}"
        assert (int(g["width"]), int(g["height"]), int(g["len"])) == (40, 36, 40 * 36) and int(s["len"]) == 64
        assert f32(g["resolution"]) == f32(p.cell_m) and [f32(v) for v in g["origin"].split(",")] == [f32(p.x_min_m), f32(p.y_min_m)]
        assert f32(s["angle_increment"]) == f32(0.02) and f32(s["angle_min"]) == f32(-0.64) + f32(0.5) * f32(0.02)
        assert f32(s["range_min"]) == 0 and f32(s["range_max"]) == f32(p.range_max_m)
    # a file the stage refuses leaves the node as it is without the variable
    obstacles.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(p, cell_m=0.0))
    msgs, grids, scans, log = _run_harness(tmp_path, "bad", m, str(tmp_path / "f.bin"), nframes,
                                           dict(cam_env, STEREONET_OBSTACLES=str(tmp_path / "bad.txt")))
    assert msgs == plain and not grids and not scans and log.count("no obstacle grid and no scan") == 1


@pytest.mark.gpu
def test_filelist_writes_the_grid_and_the_scan(model_factory, tmp_path, capsys):
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
        p = _fit(e.infer_sbs_nv12(images.sbs_from_eyes(eyes[0], eyes[1], W, H))[1].reshape(H, W), cam)
    obstacles.save_params(str(tmp_path / "ob.txt"), p)
    out = str(tmp_path / "out")
    common = ["--model", model_factory(W, H, D), "--left", lists["left"], "--right", lists["right"]]
    assert filelist.main(common + ["--out", out, "--obstacles", str(tmp_path / "ob.txt"), "--camera", "80,80,47.5,20.5,120", "--speckle", "40"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    edges = api.beam_edges(p)
    for i in range(2):
        raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)      # the final map of the chain
        occ, _, _, ranges, stats = obstacles.reference(raw, cam, p, edges=edges)
        pgm = open(os.path.join(out, f"{i}.grid.pgm"), "rb").read()
        assert pgm == b"P5\n36 40\n255\n" + obstacles.grid_image(occ).tobytes()
        rows = [l.split() for l in open(os.path.join(out, f"{i}.scan.txt")).read().splitlines()]
        assert len(rows) == 64 and [f32(r[1]) for r in rows] == list(ranges)
        assert np.allclose([float(r[0]) for r in rows], obstacles.beam_angles(p), atol=1e-6)
        near = float(ranges.min())
        assert summary["occupied"][i] == int(stats[2]) and summary["free"][i] == int(stats[3]) and int(stats[2]) + int(stats[3]) > 0
        assert summary["nearest_m"][i] == (near if np.isfinite(near) else None)
