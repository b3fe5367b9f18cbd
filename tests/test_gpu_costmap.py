"""sn_costmap on the MI355X: grid, logodds and stats equal the numpy twin's (hobot_stereonet_amd/costmap.py) byte for byte, the
twin fed the library's q and beam table, with guard bytes around every output: the clip that takes every branch of the contract
(tests/test_costmap.py asserts that it does) as one call and as seven; windows under a wave, off a multiple of 64 with an odd
height, of several workgroups and a tail, and of one cell; poses at the quantiser's limit; 1, 8 and 31 beams; 5x8 and 28x16 grids; either input absent; three
streams interleaved in one call and a reset between calls; every subset of the outputs; host mode and device mode on a caller
stream; beside inference; ground -> obstacles -> costmap on one stream from the engine's own map; argument errors; sn_destroy;
the node's topic and the filelist tool.

No tolerance appears: the contract is the same bytes."""
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

from hobot_stereonet_amd import api, costmap, ground, obstacles, synth, weights
from hobot_stereonet_amd.costmap import CostmapParams
from hobot_stereonet_amd.ground import GroundParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG, ERR_BUSY = -1, -6      # SN_ERR_ARG, SN_ERR_BUSY (include/stereonet_hip.h)
NAMES = ("grid", "logodds", "stats")
ALL = (True, True, True)


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


@functools.lru_cache(maxsize=None)
def _boundary():
    """the clip of costmap.boundary_clip with the library's q and beam table, and the twin's answer to it as one stream: shared
    by the tests and never changed"""
    p, op, poses, occ, ranges = costmap.boundary_clip()
    q, edges = api.costmap_pose_q(p, op, poses), api.beam_edges(op)
    want = costmap.Reference(p, op, edges=edges).push(q, occ, ranges)
    for a in (poses, occ, ranges, q, edges) + want:
        a.setflags(write=False)
    return p, op, poses, occ, ranges, q, edges, want


def _sizes(n, p):
    return (n * p.mw * p.mh, n * p.mw * p.mh * 2, n * 16)


def _shaped(n, p, parts):
    dt, shapes = (np.int8, np.int16, np.uint32), ((n, p.mh, p.mw), (n, p.mh, p.mw), (n, 4))
    return [None if b is None else b.view(d).reshape(s) for b, d, s in zip(parts, dt, shapes)]


def _device(torch, cm, p, poses, occ, ranges, ids=None, want=ALL, stream=0):
    """device mode: the inputs uploaded, every wanted output GUARD bytes into a buffer of 0x5a of its own -> (the three outputs
    (None where not wanted), q), after checking every byte the call must not write"""
    n = len(poses)
    d_occ = torch.from_numpy(np.array(occ)).cuda() if occ is not None else None
    d_rng = torch.from_numpy(np.array(ranges)).cuda() if ranges is not None else None
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(_sizes(n, p), want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
    q = cm.push_device(n, poses, d_occ.data_ptr() if d_occ is not None else 0, d_rng.data_ptr() if d_rng is not None else 0, ids, *ptrs,
                       stream=stream)
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
    return _shaped(n, p, parts), q


def _differing(got, want, rows=None):
    """the names of the outputs whose bytes differ from the twin's (rows: the twin's maps to compare with)"""
    bad = []
    for name, g, w_ in zip(NAMES, got, want):
        if g is None:
            continue
        w_ = w_ if rows is None else w_[rows]
        if g.dtype != w_.dtype or g.shape != w_.shape or g.tobytes() != np.ascontiguousarray(w_).tobytes():
            bad.append(name)
    return bad


@pytest.mark.gpu
def test_the_boundary_clip_as_one_call_and_as_seven(eng):
    import torch
    p, op, poses, occ, ranges, q, edges, want = _boundary()
    n = len(poses)
    with eng.costmap(op, p) as cm:
        got, q_dev = _device(torch, cm, p, poses, occ, ranges)
        assert np.array_equal(q_dev, q) and np.array_equal(cm.pose_q(poses), q) and np.array_equal(cm.pose_q(poses[3]), q[3])
        print("stats per frame:", got[2].tolist())
        assert not _differing(got, want)
        cm.reset()                                                           # the same clip again, frame by frame
        for k in range(n):
            one, _ = _device(torch, cm, p, poses[k:k + 1], occ[k:k + 1], ranges[k:k + 1])
            assert not _differing(one, want, slice(k, k + 1)), k
        cm.reset(0)                                                          # and through the host form, in two calls
        a, b = cm.push(poses[:3], occ[:3], ranges[:3]), cm.push(poses[3:], occ[3:], ranges[3:])
        assert not _differing([np.concatenate(x) for x in zip(a[:3], b[:3])], want) and np.array_equal(np.concatenate([a[3], b[3]]), q)


CONFIGS = {"1 beam, 5x8": dict(gw=5, gh=8, beams=1, angle_min_rad=-0.7, angle_increment_rad=1.4),
           "8 beams, 28x16": dict(gw=28, gh=16, beams=8, angle_min_rad=-0.8, angle_increment_rad=0.2),
           "31 beams, 5x8": dict(gw=5, gh=8, beams=31, angle_min_rad=-1.24, angle_increment_rad=0.08)}


@pytest.mark.gpu
@pytest.mark.parametrize("mw,mh", [(24, 18), (70, 33), (130, 70), (1, 1)])
def test_windows_beams_and_grids(eng, mw, mh):
    """a window under a wave, one off a multiple of 64 with an odd height, one of several workgroups and a tail, one cell; two
    streams interleaved, six frames, all outputs"""
    import torch
    for name, kw in CONFIGS.items():
        op = ObstacleParams(x_min_m=-0.5, y_min_m=-1.0, cell_m=0.25, **kw)
        p = CostmapParams(mw=mw, mh=mh, l_hit=90, l_miss=55, l_min=-130, l_max=170, clear_margin_m=0.2, clear_min_m=0.3, clear_max_m=0.0)
        poses, occ, ranges = costmap.synthetic_clip(p, op, 6, seed=mw + op.beams)
        ids = [0, 1, 1, 0, 0, 1]
        twin = costmap.Reference(p, op, 2, edges=api.beam_edges(op))
        with eng.costmap(op, p, streams=2) as cm:
            got, q = _device(torch, cm, p, poses, occ, ranges, ids)
            want = twin.push(q, occ, ranges, ids)
            assert not _differing(got, want), (name, got[2].tolist(), want[2].tolist())
        if mw > 1:      # the clip does something: hits, clears by the grid and by rays alone, a window that moves
            tot = {k: sum(f[k] for f in twin.frames) for k in ("hit", "clear_occ", "clear_ray")}
            assert all(v > 0 for v in tot.values()) and any(f["prev"] not in (None, f["origin"]) for f in twin.frames), (name, tot)


@pytest.mark.gpu
def test_poses_at_the_far_limit(eng):
    """|x| * k256 = 2^30 exactly, the largest translation the quantiser takes, in both signs: the kernel's 32-bit cell arithmetic
    (cx * 256 + 128 reaches 2^30 + 2^15 here) gives the twin's int64 bytes"""
    import torch
    op = ObstacleParams(x_min_m=-0.5, y_min_m=-1.0, cell_m=0.25, **CONFIGS["8 beams, 28x16"])
    p = CostmapParams(mw=130, mh=70, l_hit=90, l_miss=55, l_min=-130, l_max=170, clear_margin_m=0.2, clear_min_m=0.3, clear_max_m=0.0)
    lim = 2.0 ** 30 / costmap.units(p, op).k256
    _, occ, ranges = costmap.synthetic_clip(p, op, 4, seed=9)
    poses = np.array([[lim, -lim, 0.7], [lim - 0.75, -lim + 0.5, 2.5], [-lim, lim, -1.2], [-lim + 0.25, lim - 0.5, 0.0]])
    twin = costmap.Reference(p, op, edges=api.beam_edges(op))
    with eng.costmap(op, p) as cm:
        got, q = _device(torch, cm, p, poses, occ, ranges)
        assert q[0, 0] == 1 << 30 and q[0, 1] == -(1 << 30) and q[2, 0] == -(1 << 30) and q[2, 1] == 1 << 30
        want = twin.push(q, occ, ranges)
        assert not _differing(got, want), (got[2].tolist(), want[2].tolist())
    assert all(f["hit"] > 0 and f["clear_ray"] > 0 for f in twin.frames) and twin.frames[1]["prev"] != twin.frames[1]["origin"]
    assert twin.frames[2]["scrolled"] > 0


@pytest.mark.gpu
def test_either_input_absent(eng):
    import torch
    p, op, poses, occ, ranges, q, edges, _ = _boundary()
    for o, r in ((occ, None), (None, ranges)):
        with eng.costmap(op, p) as cm:
            got, _ = _device(torch, cm, p, poses, o, r)
            want = costmap.Reference(p, op, edges=edges).push(q, o, r)
            assert not _differing(got, want) and want[2][:, 2 if o is not None else 3].all(), "occ only" if r is None else "ranges only"
    # ... and where the parameters leave one out, the pointer is not read
    for kw, o, r in ((dict(beams=0), occ, ranges), (dict(gw=0, gh=0), occ, ranges)):
        op2 = dataclasses.replace(op, **kw)
        with eng.costmap(op2, p) as cm:
            got, _ = _device(torch, cm, p, poses, o if op2.gw else None, r if op2.beams else None)
            want = costmap.Reference(p, op2, edges=edges if op2.beams else None).push(q, o, r)
            assert not _differing(got, want), kw


@pytest.mark.gpu
def test_three_streams_interleaved_and_a_reset_mid_sequence(eng):
    import torch
    p, op, poses, occ, ranges, q, edges, _ = _boundary()
    # ten maps: the clip's frames dealt to three streams that each start somewhere else in it
    order = [0, 3, 5, 1, 4, 6, 2, 5, 0, 3]
    ids = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    po, oc, rg, qq = poses[order], occ[order], ranges[order], q[order]
    twin = costmap.Reference(p, op, 3, edges=edges)
    with eng.costmap(op, p, streams=3) as cm:
        got, _ = _device(torch, cm, p, po, oc, rg, ids)
        assert not _differing(got, twin.push(qq, oc, rg, ids))
        cm.reset(1)
        twin.reset(1)
        got, _ = _device(torch, cm, p, po[:6], oc[:6], rg[:6], ids[:6])
        want = twin.push(qq[:6], oc[:6], rg[:6], ids[:6])
        assert not _differing(got, want)
        fresh = [f for f in twin.frames[-6:] if f["stream"] == 1][0]
        assert fresh["prev"] is None and fresh["scrolled"] == 0 and want[2][1, 0] == fresh["born"]      # stream 1 began anew, the others went on
        assert all(f["prev"] is not None for f in twin.frames[-6:] if f["stream"] != 1)
        cm.reset()
        twin.reset()
        got, _ = _device(torch, cm, p, po[6:], oc[6:], rg[6:], ids[6:])
        assert not _differing(got, twin.push(qq[6:], oc[6:], rg[6:], ids[6:]))


@pytest.mark.gpu
def test_every_subset_of_the_outputs_in_both_memory_modes(eng):
    import torch
    p, op, poses, occ, ranges, q, edges, want = _boundary()
    side = torch.cuda.Stream()
    with eng.costmap(op, p) as cm:
        for sub in itertools.product((False, True), repeat=3):
            if not any(sub):
                continue
            for stream in (0, side.cuda_stream):                               # blocking | a caller stream
                cm.reset()
                got, _ = _device(torch, cm, p, poses[:4], occ[:4], ranges[:4], want=sub, stream=stream)
                more, _ = _device(torch, cm, p, poses[4:], occ[4:], ranges[4:], stream=stream)      # the state went on whatever was asked for
                assert not _differing(got, want, slice(0, 4)) and not _differing(more, want, slice(4, 7)), (sub, stream)
            cm.reset()                                                         # host mode
            got = cm.push(poses, occ, ranges, want=sub)
            assert [g is not None for g in got[:3]] == list(sub) and not _differing(got[:3], want), sub


@pytest.mark.gpu
def test_costmap_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread pushes clips (ctypes drops the GIL): the maps of both equal the serial run's."""
    p, op, poses, occ, ranges, q, edges, want = _boundary()
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=MAX_BATCH) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, rounds = [], []
        with e.costmap(op, p) as cm:
            def work():
                try:
                    for _ in range(12):
                        cm.reset()
                        if _differing(cm.push(poses, occ, ranges)[:3], want):
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


def _scene_params(raw, cam, fit_ground=False, out_scale=None):
    """obstacle and costmap parameters (and with fit_ground the ground stage's, first) that make something of the engine's own
    maps, whatever its synthetic weights give: the widest gate and the narrowest of a few inlier bands that finds a plane in
    map 0, an obstacle grid fitted to the points under that plane's mount (else under a level mount)"""
    kw = {} if out_scale is None else dict(out_scale=out_scale)
    gp, level = None, obstacles.mount(t=(0.0, 0.0, 0.3))
    for tol in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0) if fit_ground else ():
        cand = GroundParams(hypotheses=512, seed=2, refits=2, tol_px=tol, min_inliers=W * (H // 2) // 10, min_area=16, max_tilt_rad=1.5,
                            height_min_m=0.01, height_max_m=100.0)
        rec = ground.reference(raw[0], cam, cand, gate_q16=api.ground_gate(cam, cand, W, H), labels=False, **kw)[0]
        if rec["flags"] & ground.FOUND:
            gp, level = cand, tuple(float(v) for v in rec["base_from_cam"])
            break
    assert gp is not None or not fit_ground, "no plane in the engine's map"
    xb, yb, zb = obstacles.base_points(raw, cam, ObstacleParams(base_from_cam=level), **kw)
    ok = np.isfinite(xb)
    assert ok.sum() > 500, "the engine's maps hold too few measurements"
    pc = lambda a, v: float(np.float32(np.percentile(a[ok].astype(np.float64), v)))      # noqa: E731
    x0, x1, y0, y1 = pc(xb, 5), pc(xb, 95), pc(yb, 5), pc(yb, 95)
    cell = float(np.float32(max((x1 - x0) / 28, (y1 - y0) / 16, 1e-3)))
    op = ObstacleParams(base_from_cam=level, x_min_m=x0, y_min_m=y0, cell_m=cell, gw=28, gh=16, z_floor_m=-1e3, z_lo_m=pc(zb, 50), z_hi_m=1e3,
                        min_obstacle_hits=1, min_ground_hits=1, beams=31, angle_min_rad=-0.62, angle_increment_rad=0.04, range_min_m=0.0,
                        range_max_m=float(np.float32(4 * abs(x1) + 1)))
    return gp, op, CostmapParams(mw=70, mh=33, l_hit=100, l_miss=60, l_min=-150, l_max=250, clear_margin_m=cell, clear_min_m=0.0, clear_max_m=0.0)


@pytest.mark.gpu
def test_end_to_end_on_the_device_from_the_engines_own_map(eng):
    """sn_infer_batch -> sn_ground_from_raw -> sn_obstacles_from_raw_mounts -> sn_costmap_push on one stream: nothing crosses to
    the host in between"""
    import torch
    n = 4
    x = np.stack([synth.model_input_i8(W, H, D, 20 + k) for k in range(n)])
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    raw_host = np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)])
    gp, op, p = _scene_params(raw_host, cam, True, eng.out_scale)
    poses = np.array([[0.0, 0.0, 0.0], [op.cell_m * 1.5, 0.0, 0.1], [op.cell_m * 3.0, op.cell_m, 0.2], [op.cell_m * 3.0, -op.cell_m, -0.4]])
    d_in = torch.from_numpy(x).cuda()
    d_raw = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    d_rec = torch.zeros(n * ground.RECORD.itemsize, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n * op.gw * op.gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_rng = torch.full((n * op.beams,), 7.0, dtype=torch.float32, device="cuda")
    outs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, p)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with eng.costmap(op, p) as cm:
        eng.infer_device(n, d_in.data_ptr(), d_raw.data_ptr(), 0, stream=st.cuda_stream)
        eng.ground_device(n, d_raw.data_ptr(), cam, gp, d_rec.data_ptr(), 0, stream=st.cuda_stream)
        eng.obstacles_device(n, d_raw.data_ptr(), cam, op, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr(), stream=st.cuda_stream,
                             mounts_ptr=d_rec.data_ptr() + 4 * ground.MOUNT_OFFSET_FLOATS, mount_stride=ground.RECORD_FLOATS)
        q = cm.push_device(n, poses, d_occ.data_ptr(), d_rng.data_ptr(), None, *[o.data_ptr() for o in outs], stream=st.cuda_stream)
        torch.cuda.synchronize()
    raw = d_raw.cpu().numpy()
    assert np.array_equal(raw, raw_host)
    # the twins of the three stages, each fed what the chain says it is fed
    rec = ground.reference(raw, cam, gp, gate_q16=api.ground_gate(cam, gp, W, H), labels=False, out_scale=eng.out_scale)[0]
    assert np.array_equal(d_rec.cpu().numpy().view(ground.RECORD)["base_from_cam"].view(np.uint32), rec["base_from_cam"].view(np.uint32))
    edges = api.beam_edges(op)
    occ = np.stack([obstacles.reference(raw[k], cam, dataclasses.replace(op, base_from_cam=tuple(rec["base_from_cam"][k])), edges=edges,
                                        out_scale=eng.out_scale)[0] for k in range(n)])
    rng = np.stack([obstacles.reference(raw[k], cam, dataclasses.replace(op, base_from_cam=tuple(rec["base_from_cam"][k])), edges=edges,
                                        out_scale=eng.out_scale)[3] for k in range(n)])
    assert d_occ.cpu().numpy().view(np.int8).tobytes() == occ.tobytes() and d_rng.cpu().numpy().view(np.uint32).tobytes() == rng.view(np.uint32).tobytes()
    twin = costmap.Reference(p, op, edges=edges)
    want = twin.push(q, occ, rng)
    print("end to end stats:", want[2].tolist())
    assert want[2][:, 2].sum() > 0 and want[2][:, 3].sum() > 0 and sum(f["clear_ray"] for f in twin.frames) > 0      # a scene, not an empty map
    assert not _differing(_shaped(n, p, [o.cpu().numpy() for o in outs]), want)


@pytest.mark.gpu
def test_argument_errors_change_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    p, op, poses, occ, ranges, q, edges, want = _boundary()
    n = len(poses)
    c_op, c_p = api.obstacle_params(op), api.costmap_params(p)

    def failed(rc, name):
        msg = lib.sn_last_error(hnd).decode()
        return rc == ERR_ARG and msg.startswith(name + ": ") and len(msg) > len(name) + 2

    # sn_costmap_create (the parameter rules are tried without a device in tests/test_costmap.py)
    c = C.c_void_p()
    for streams in (0, -1, MAX_BATCH + 1):
        assert failed(lib.sn_costmap_create(hnd, streams, C.byref(c_op), C.byref(c_p), C.byref(c)), "sn_costmap_create"), streams
    assert failed(lib.sn_costmap_create(hnd, 1, None, C.byref(c_p), C.byref(c)), "sn_costmap_create")
    assert failed(lib.sn_costmap_create(hnd, 1, C.byref(c_op), None, C.byref(c)), "sn_costmap_create")
    assert failed(lib.sn_costmap_create(hnd, 1, C.byref(c_op), C.byref(c_p), None), "sn_costmap_create")
    for kw in (dict(mw=0), dict(mh=4097), dict(l_hit=0), dict(l_miss=40000), dict(l_min=0), dict(l_max=-1), dict(clear_margin_m=-1.0),
               dict(clear_max_m=math.nan), dict(clear_min_m=math.inf)):
        bad_p = api.costmap_params(dataclasses.replace(p, **kw))
        assert failed(lib.sn_costmap_create(hnd, 1, C.byref(c_op), C.byref(bad_p), C.byref(c)), "sn_costmap_create"), kw
    for kw in (dict(cell_m=0.0), dict(cell_m=math.nan), dict(x_min_m=math.inf), dict(y_min_m=math.nan), dict(gw=0), dict(gh=5000), dict(beams=-2),
               dict(beams=4097), dict(angle_increment_rad=0.5), dict(gw=0, gh=0, beams=0)):
        bad_op = api.obstacle_params(dataclasses.replace(op, **kw))
        assert failed(lib.sn_costmap_create(hnd, 1, C.byref(bad_op), C.byref(c_p), C.byref(c)), "sn_costmap_create"), kw
    assert not c.value
    with eng.costmap(op, dataclasses.replace(p, mw=1, mh=4096, l_hit=32767, l_miss=32767, l_min=-32767, l_max=32767, clear_margin_m=3e38)):
        pass                                                                     # the bounds themselves are allowed

    cm = eng.costmap(op, p, streams=2)
    sizes = _sizes(MAX_BATCH, p)
    d_occ, d_rng = torch.from_numpy(occ.copy()).cuda(), torch.from_numpy(ranges.copy()).cuda()
    bufs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [b.data_ptr() for b in bufs]
    q_out = np.full((MAX_BATCH, 6), 77, np.int32)
    torch.cuda.synchronize()

    def call(n=1, ids=None, ps=poses, o=None, r=None, out=None, qo=q_out, mem=api.SN_MEM_DEVICE, obj=None):
        ps = None if ps is None else np.ascontiguousarray(ps, np.float64)
        ids = None if ids is None else np.asarray(ids, np.int32)
        out = ptr if out is None else out
        return lib.sn_costmap_push(cm._c if obj is None else obj, n, api._np_ptr(ids), api._np_ptr(ps), (d_occ.data_ptr() if o is None else o) or None,
                                   (d_rng.data_ptr() if r is None else r) or None, *[v or None for v in out], api._np_ptr(qo), mem, None)

    far = 2.0 ** 30 / costmap.units(p, op).k256 * 1.001
    bad = {"n = 0": dict(n=0), "n > max_batch": dict(n=MAX_BATCH + 1), "null poses": dict(ps=None), "bad mem": dict(mem=7),
           "no outputs": dict(out=[0, 0, 0]), "neither input": dict(o=0, r=0),
           "id too large": dict(n=2, ids=[0, 2]), "id negative": dict(n=2, ids=[-1, 0]),
           "x nan": dict(ps=[[math.nan, 0, 0]]), "y inf": dict(ps=[[0, math.inf, 0]]), "yaw nan": dict(ps=[[0, 0, math.nan]]),
           "x too far": dict(ps=[[far, 0, 0]]), "second pose bad": dict(n=2, ps=[[0, 0, 0], [0, -far, 0]]),
           "logodds odd": dict(out=[ptr[0], ptr[1] + 1, ptr[2]]), "stats misaligned": dict(out=[ptr[0], ptr[1], ptr[2] + 2]),
           "occ overlaps grid": dict(out=[d_occ.data_ptr() + 8, ptr[1], ptr[2]]),
           "ranges overlaps logodds": dict(out=[ptr[0], d_rng.data_ptr(), ptr[2]]),
           "grid overlaps logodds": dict(out=[ptr[1] + 2, ptr[1], ptr[2]]), "logodds overlaps stats": dict(out=[ptr[0], ptr[2], ptr[2] + 4])}
    for name, kw in bad.items():
        assert failed(call(**kw), "sn_costmap_push"), name
    assert lib.sn_costmap_push(None, 1, None, poses.ctypes.data, d_occ.data_ptr(), None, ptr[0], None, None, None, api.SN_MEM_DEVICE, None) == ERR_ARG
    assert failed(lib.sn_costmap_reset(cm._c, 2), "sn_costmap_reset") and failed(lib.sn_costmap_reset(cm._c, -2), "sn_costmap_reset")
    assert lib.sn_costmap_pose_q(cm._c, None, q_out.ctypes.data) == ERR_ARG and lib.sn_costmap_pose_q(None, poses.ctypes.data, q_out.ctypes.data) == ERR_ARG
    with pytest.raises(api.StereoNetError):
        cm.push(poses, occ[:2], ranges)
    with pytest.raises(api.StereoNetError):
        cm.push(poses, occ, ranges, stream_of=[0])
    torch.cuda.synchronize()
    # nothing was written and no state changed: the first good call is a first frame, the rest of the clip continues stream 0 as
    # if the failed calls had not been made, and stream 1 is still fresh
    assert all(bool((b == 0x5a).all()) for b in bufs) and np.all(q_out == 77)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((bufs[0][p.mw * p.mh:] == 0x5a).all()) and bool((bufs[1][2 * p.mw * p.mh:] == 0x5a).all()) and bool((bufs[2][16:] == 0x5a).all())
    assert np.all(q_out[1:] == 77) and np.array_equal(q_out[0], q[0])
    first = _shaped(1, p, [b.cpu().numpy()[:s // MAX_BATCH] for b, s in zip(bufs, sizes)])
    assert not _differing(first, want, slice(0, 1))
    rest, _ = _device(torch, cm, p, poses[1:], occ[1:], ranges[1:])
    assert not _differing(rest, want, slice(1, n))
    other, _ = _device(torch, cm, p, poses, occ, ranges, [1] * n)
    assert not _differing(other, want)
    cm.close()


@pytest.mark.gpu
def test_destroy_is_refused_while_a_costmap_lives(model_factory):
    p, op, poses, occ, ranges, q, edges, want = _boundary()
    eng = api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH)
    lib, hd = eng._lib, eng._h
    x = synth.model_input_i8(W, H, D, 3)
    before = eng.infer(x)[1]
    cm = eng.costmap(op, p)
    half = cm.push(poses[:3], occ[:3], ranges[:3])
    assert lib.sn_destroy(hd) == ERR_BUSY and "costmap" in lib.sn_last_error(hd).decode()
    with pytest.raises(api.StereoNetError):
        eng.close()
    more = cm.push(poses[3:], occ[3:], ranges[3:])                              # both are as usable as before
    assert not _differing([np.concatenate(v) for v in zip(half[:3], more[:3])], want) and np.array_equal(eng.infer(x)[1], before)
    cm.close()
    cm.close()
    eng.close()
    assert not eng._h.value


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra, poses=None):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    args = [os.path.join(COMPAT, "build", "costmap_harness"), model, frames, str(W), str(H), str(nframes), prefix]
    if poses is not None:
        path = str(tmp_path / f"{tag}.poses")
        with open(path, "w") as f:
            f.write("".join(f"{float(x)!r} {float(y)!r} {float(yaw)!r}\n" for x, y, yaw in poses))
        args.append(path)
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    maps = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("costmap ")]
    order = [l.split()[0] for l in lines if l.split()[0] in ("grid", "scan", "costmap")]
    return maps, order, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_costmap(weights_blob, tmp_path):
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 4
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(str(tmp_path / "f.bin"))
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0, z_min_m=0.05)
    with api.StereoNetHIP(m) as e:
        _, op, p = _scene_params(e.infer_sbs_nv12(sbs)[1].reshape(1, H, W), cam)
    op = dataclasses.replace(op, frame="base_footprint")
    p = dataclasses.replace(p, frame="map")
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), p)
    cam_env = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0", "STEREONET_OBSTACLES": str(tmp_path / "ob.txt")}
    f_bin = str(tmp_path / "f.bin")
    none, order, _ = _run_harness(tmp_path, "off", m, f_bin, nframes, cam_env)
    assert not none and order == ["grid", "scan"] * nframes                     # unset: nothing on the topic
    poses = np.array([[0.0, 0.0, 0.0], [2 * op.cell_m, 0.0, 0.1], [2 * op.cell_m, -op.cell_m, math.pi / 2], [-30 * op.cell_m, 7 * op.cell_m, -2.0]])
    edges = api.beam_edges(op)
    for tag, ps in (("posed", poses), ("still", None)):                          # without SetBasePose: the origin for every frame
        maps, order, log = _run_harness(tmp_path, tag, m, f_bin, nframes, dict(cam_env, STEREONET_COSTMAP=str(tmp_path / "cm.txt")), ps)
        assert len(maps) == nframes and order == ["grid", "scan", "costmap"] * nframes and "/stereonet_costmap" in log
        q = api.costmap_pose_q(p, op, poses if ps is not None else np.zeros((nframes, 3)))
        occ = np.stack([np.fromfile(str(tmp_path / f"{tag}.{k}.grid"), np.int8).reshape(op.gh, op.gw) for k in range(nframes)])
        rng = np.stack([np.fromfile(str(tmp_path / f"{tag}.{k}.scan"), np.float32) for k in range(nframes)])
        twin = costmap.Reference(p, op, edges=edges)
        want = twin.push(q, occ, rng)[0]
        assert (want >= 0).any() and sum(f["hit"] + f["clear_ray"] for f in twin.frames) > 0
        for k in range(nframes):
            assert open(tmp_path / f"{tag}.{k}.costmap", "rb").read() == want[k].tobytes(), (tag, k)
            g = maps[k]
            assert g["frame_id"] == "map" and g["stamp"] == f"7.{1000 + k}" and (int(g["width"]), int(g["height"]), int(g["len"])) == (70, 33, 70 * 33)
            assert np.float32(g["resolution"]) == np.float32(op.cell_m)
            cell = float(np.float32(op.cell_m))
            assert [float(v) for v in g["origin"].split(",")] == [float(np.float64(f"{int(q[k, 4]) * cell:.9g}")), float(np.float64(f"{int(q[k, 5]) * cell:.9g}"))]
    # without the obstacle stage, or with a file the stage refuses, the node is as it is without the variable
    env = {k: v for k, v in cam_env.items() if k != "STEREONET_OBSTACLES"}
    maps, order, log = _run_harness(tmp_path, "alone", m, f_bin, nframes, dict(env, STEREONET_COSTMAP=str(tmp_path / "cm.txt")))
    assert not maps and not order and log.count("requires STEREONET_OBSTACLES") == 1 and log.count("no costmap") == 1
    costmap.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(p, l_min=5))
    maps, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, dict(cam_env, STEREONET_COSTMAP=str(tmp_path / "bad.txt")))
    assert not maps and order == ["grid", "scan"] * nframes and log.count("no costmap") == 1


@pytest.mark.gpu
def test_filelist_writes_the_costmap(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    rng = np.random.default_rng(11)
    n, lists = 3, {}
    for eye in ("left", "right"):
        paths = []
        for i in range(n):
            path = str(tmp_path / f"{eye}{i}.ppm")
            images.write_ppm(path, rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            paths.append(path)
        lists[eye] = str(tmp_path / f"{eye}.list")
        with open(lists[eye], "w") as f:
            f.write("\n".join(paths) + "\n")
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    model = model_factory(W, H, D)
    with api.StereoNetHIP(model) as e:
        eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}0.ppm"))) for eye in ("left", "right")]
        _, op, p = _scene_params(e.infer_sbs_nv12(images.sbs_from_eyes(eyes[0], eyes[1], W, H))[1].reshape(1, H, W), cam)
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), p)
    poses = np.array([[0.0, 0.0, 0.0], [op.cell_m, 0.0, 0.2], [3 * op.cell_m, -op.cell_m, -0.3]])
    (tmp_path / "poses.txt").write_text("# x y yaw\n" + "".join(f"{float(x)!r} {float(y)!r} {float(yaw)!r}\n" for x, y, yaw in poses))
    common = ["--model", model, "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120"]
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--costmap", str(tmp_path / "cm.txt")])      # requires --obstacles
    capsys.readouterr()
    edges = api.beam_edges(op)
    for tag, arg, ps in (("posed", f"{tmp_path / 'cm.txt'},{tmp_path / 'poses.txt'}", poses), ("still", str(tmp_path / "cm.txt"), np.zeros((n, 3)))):
        out = str(tmp_path / tag)
        assert filelist.main(common + ["--out", out, "--obstacles", str(tmp_path / "ob.txt"), "--costmap", arg]) == 0
        summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        twin = costmap.Reference(p, op, edges=edges)
        q = api.costmap_pose_q(p, op, ps)
        for i in range(n):
            raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)
            occ, _, _, ranges, _ = obstacles.reference(raw, cam, op, edges=edges)
            grid, _, stats = twin.push(q[i:i + 1], occ[None], ranges[None])
            pgm = open(os.path.join(out, f"{i}.costmap.pgm"), "rb").read()
            assert pgm == f"P5\n{p.mh} {p.mw}\n255\n".encode() + costmap.grid_image(grid[0]).tobytes(), (tag, i)
            assert [summary["costmap"][k][i] for k in ("known", "occupied", "hit", "cleared")] == stats[0].tolist() and stats[0, 0] > 0
        assert summary["frames"] == n and len(summary["occupied"]) == n          # the obstacle stage's own keys are as before
