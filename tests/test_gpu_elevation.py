"""sn_elevation on the MI355X: trav, hi, lo, rise and stats equal the numpy twin's (hobot_stereonet_amd/elevation.py) byte for
byte, the twin fed the library's q, with guard bytes around every output: a clip as one call, frame by frame and through the
host form; on a caller stream; windows next to the verdict kernel's 64 x 16 tile; maps that are no multiple of the wave, at step
1 and 2; streams interleaved; every point in one cell, an all-zero map, a mount that is not finite, known cells on the window's
border with radius 1 and 3, a jump of more than a window; every subset of one output; mounts read from device memory with a
stride; argument errors that leave outputs and state untouched; sn_destroy.

No tolerance appears: the contract is the same bytes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from hobot_stereonet_amd import api, obstacles
from hobot_stereonet_amd import elevation as el
from hobot_stereonet_amd.elevation import ElevationParams
from hobot_stereonet_amd.pointcloud import Camera

W, H, D = 96, 64, 48
MAX_BATCH = 6
GUARD = 16
ERR_ARG, ERR_BUSY = -1, -6      # SN_ERR_ARG, SN_ERR_BUSY (include/stereonet_hip.h)
NAMES = ("trav", "hi", "lo", "rise", "stats")
DTYPES = (np.int8, np.int16, np.int16, np.uint16, np.uint32)
ALL = (True,) * 5
CAM = Camera(fx=40.0, fy=40.0, baseline_mm=120.0)
P = ElevationParams(mw=70, mh=33, cell_m=0.2, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=2, alpha=96, max_step_mm=70, radius=2)


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _sizes(n, p):
    c = n * p.mw * p.mh
    return (c, 2 * c, 2 * c, 2 * c, n * 16)


def _shaped(n, p, parts):
    shapes = ((n, p.mh, p.mw),) * 4 + ((n, 4),)
    return [None if b is None else b.view(d).reshape(s) for b, d, s in zip(parts, DTYPES, shapes)]


def _device(torch, ev, p, poses, raw, cam, mounts=None, stride=12, ids=None, want=ALL, stream=0):
    """device mode: the maps (and mounts, `stride` floats apart) uploaded, every wanted output GUARD bytes into a buffer of 0x5a
    of its own -> (the five outputs (None where not wanted), q), after checking every byte the call must not write"""
    n = len(poses)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw, np.int32)).cuda()
    d_m = None
    if mounts is not None:
        wide = np.full((n, stride), 7.0, np.float32)
        wide[:, :12] = np.asarray(mounts, np.float32).reshape(n, 12)
        d_m = torch.from_numpy(wide).cuda()
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(_sizes(n, p), want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
    q = ev.push_device(n, poses, d_raw.data_ptr(), cam, d_m.data_ptr() if d_m is not None else 0, stride, ids, *ptrs, stream=stream)
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
def test_a_clip_as_one_call_frame_by_frame_through_the_host_and_on_a_caller_stream(eng):
    import torch
    _, raw = el.synthetic_clip(P, W, H, CAM, 3, seed=21)
    poses = np.array([[0.0, 0.0, 0.0], [0.9, 0.3, 0.4], [-1.5, -0.6, -0.5]])      # forward and to the left, then back by twelve cells
    with eng.elevation(P) as ev:
        got, q = _device(torch, ev, P, poses, raw, CAM)
        assert np.array_equal(q, api.elevation_pose_q(P, poses)) and np.array_equal(ev.pose_q(poses), q) and np.array_equal(ev.pose_q(poses[1]), q[1])
        twin = el.Reference(P)
        want = twin.push(q, raw, CAM)
        print("stats per frame:", got[4].tolist(), "branches:", [{k: v for k, v in f.items() if k in ("born", "up", "down", "scrolled")} for f in twin.frames])
        assert not _differing(got, want)
        assert {-1, 0, 100} <= set(np.unique(want[0]).tolist()) and sum(f["scrolled"] for f in twin.frames) and sum(f["up"] + f["down"] for f in twin.frames)
        ev.reset()                                                           # the same clip again, frame by frame
        for k in range(3):
            one, _ = _device(torch, ev, P, poses[k:k + 1], raw[k:k + 1], CAM)
            assert not _differing(one, want, slice(k, k + 1)), k
        ev.reset(0)                                                          # through the host form, in two calls
        a, b = ev.push(poses[:1], raw[0], CAM), ev.push(poses[1:], raw[1:], CAM)
        assert not _differing([np.concatenate(x) for x in zip(a[:5], b[:5])], want) and np.array_equal(np.concatenate([a[5], b[5]]), q)
        ev.reset()                                                           # on a stream of the caller's: enqueued only
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            on_stream, _ = _device(torch, ev, P, poses, raw, CAM, stream=s.cuda_stream)
        assert not _differing(on_stream, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mw,mh", [(1, 1), (1, 7), (65, 17), (33, 100)])
def test_windows_next_to_the_verdict_tile(eng, mw, mh):
    """one cell, one column, one past the 64 x 16 tile both ways, and seven tiles high with a partial one; two streams x two frames,
    every radius"""
    import torch
    for radius in (1, 2, 3):
        # the small windows get cells of 3 m, so that the robot's own cell holds the ground ahead of it
        p = dataclasses.replace(P, mw=mw, mh=mh, radius=radius, min_points=1, cell_m=0.2 if mw * mh > 100 else 3.0)
        poses, raw = el.synthetic_clip(p, W, H, CAM, 4, seed=mw + radius, step_cells=2.5 if mw * mh > 100 else 0.4)
        ids = [0, 1, 1, 0]
        with eng.elevation(p, streams=2) as ev:
            got, q = _device(torch, ev, p, poses, raw, CAM, ids=ids)
            want = el.Reference(p, 2).push(q, raw, CAM, stream_of=ids)
            assert not _differing(got, want), radius
            assert want[4][:, 0].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,step", [(96, 64, 1), (96, 64, 2), (5, 3, 1), (1, 1, 1)])
def test_maps_that_are_no_multiple_of_the_wave(model_factory, w, h, step):
    import torch
    cam = dataclasses.replace(CAM, fx=0.4 * max(w, 2), fy=0.4 * max(w, 2), step=step, cx=w / 2.0, cy=0.0 if h < 4 else h / 2.0)
    p = dataclasses.replace(P, mw=21, mh=18, cell_m=0.25, min_points=1, radius=1)
    with api.StereoNetHIP(model_factory(w, h, 16), max_batch=3) as e, e.elevation(p) as ev:
        for n in (1, 3):                                                     # n = 1, then a 3-frame clip on top of it
            poses, raw = el.synthetic_clip(p, w, h, cam, n, seed=w + n)
            raw[raw <= 0] = 0 if w > 5 else 900                             # the tiny maps keep all of their few samples
            if n == 1:
                twin = el.Reference(p)
            got, q = _device(torch, ev, p, poses, raw, cam)
            want = twin.push(q, raw, cam)
            assert not _differing(got, want), n
            assert want[4][:, 3].min() > 0, "no point was used"


@pytest.mark.gpu
def test_collisions_and_degenerate_inputs(eng):
    import torch
    # every point in one cell: a cell of 64 m (and a window of one cell, and of 3 x 3 with the robot in the middle)
    _, raw = el.synthetic_clip(P, W, H, CAM, 2, seed=5)
    poses = np.array([[10.0, 10.0, 0.0], [10.5, 10.2, 0.3]])      # well inside the world cell [0, 64) x [0, 64)
    for mw, mh in ((1, 1), (3, 3)):
        p = dataclasses.replace(P, mw=mw, mh=mh, cell_m=64.0, range_max_m=30.0)
        with eng.elevation(p) as ev:
            got, q = _device(torch, ev, p, poses, raw, CAM)
            want = el.Reference(p).push(q, raw, CAM)
            assert not _differing(got, want) and (want[4][:, 2] == 1).all() and want[4][0, 3] > 1000
    # an all-zero map fuses nothing and leaves the first frame's cells; then a jump of more than a window forgets them
    far = np.array([[0.3, -0.2, 0.1], [0.3, -0.2, 0.1], [0.3 + 2 * P.mw * P.cell_m, -0.2, 0.1]])
    maps = np.stack([raw[0], np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)])
    with eng.elevation(P) as ev:
        got, q = _device(torch, ev, P, far, maps, CAM)
        want = el.Reference(P).push(q, maps, CAM)
        assert not _differing(got, want)
        assert want[4][0, 0] > 0 and want[4][1].tolist() == [want[4][0, 0], want[4][0, 1], 0, 0] and want[4][2].tolist() == [0, 0, 0, 0]
        assert (got[0][2] == -1).all() and (got[1][2] == el.UNKNOWN).all() and not got[3][2].any()
    # a mount that is not finite, through `mounts` (48 floats apart): nothing is fused, the state stays
    mounts = np.asarray([obstacles.mount(0.0, 0.15, (0.0, 0.0, 0.45)), (np.nan,) * 12, obstacles.mount(0.1, 0.1, (0.1, 0.0, 0.4))], np.float32)
    mounts[1, 5] = 1.0
    still = np.array([[0.0, 0.0, 0.0]] * 3)
    maps = np.stack([raw[0], raw[1], raw[1]])
    with eng.elevation(P) as ev:
        got, q = _device(torch, ev, P, still, maps, CAM, mounts=mounts, stride=48)
        want = el.Reference(P).push(q, maps, CAM, mounts)
        assert not _differing(got, want)
        assert want[4][1, 2] == 0 and want[4][1, 3] == 0 and np.array_equal(got[1][1], got[1][0]) and want[4][2, 2] > 0
        ev.reset()
        host = ev.push(still, maps, CAM, mounts)
        assert not _differing(host[:5], want)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 3])
def test_known_cells_on_the_windows_border(eng, radius):
    """a window that lies wholly on the ground in front of the robot, so its border cells are known and their neighbourhoods are
    clipped; a smooth floor 0.45 m below a level camera that sits 1.2 m behind the base frame's origin"""
    import torch
    p = dataclasses.replace(P, mw=9, mh=7, cell_m=0.1, radius=radius, min_points=1, max_step_mm=25, alpha=256,
                            base_from_cam=obstacles.mount(0.0, 0.0, (-1.2, 0.0, 0.45)))
    raw = el.terrain_map(W, H, CAM, 0.45, 30.0, seed=3, rough_m=0.0, holes=0.0)[None]
    with eng.elevation(p) as ev:
        got, q = _device(torch, ev, p, [(0.0, 0.0, 0.0)], raw, CAM)
        want = el.Reference(p).push(q, raw, CAM)
        assert not _differing(got, want)
        known = want[1][0] != el.UNKNOWN
        print("known border cells:", int(known[0].sum() + known[-1].sum() + known[:, 0].sum() + known[:, -1].sum()))
        assert known[0].any() and known[-1].any() and known[:, 0].any() and known[:, -1].any() and known[0, 0] and known[-1, -1]
        assert (want[0][0][known] == 0).all() and np.abs(want[1][0][known].astype(int)).max() <= 2      # the floor is z = 0, and drivable


@pytest.mark.gpu
def test_every_output_alone_and_the_scratch_planes(eng):
    import torch
    poses, raw = el.synthetic_clip(P, W, H, CAM, 2, seed=8)
    want = None
    for only in range(5):
        flags = tuple(i == only for i in range(5))
        with eng.elevation(P) as ev:
            got, q = _device(torch, ev, P, poses, raw, CAM, want=flags)
            want = want or el.Reference(P).push(q, raw, CAM)
            assert not _differing(got, want), NAMES[only]
            host = ev.push(poses, raw, CAM, want=flags)      # a second pair of frames on top, through the host form
            again = el.Reference(P)
            again.push(q, raw, CAM)
            assert not _differing(host[:5], again.push(q, raw, CAM)), NAMES[only]


@pytest.mark.gpu
def test_refused_calls_leave_outputs_and_state_untouched(eng):
    import torch
    lib = eng._lib
    poses, raw = el.synthetic_clip(P, W, H, CAM, 3, seed=13)
    n = 2
    cam = api._sn_camera(CAM, W, H)
    with eng.elevation(P, streams=2) as ev:
        first, q = _device(torch, ev, P, poses[:1], raw[:1], CAM)
        twin = el.Reference(P, 2)
        twin.push(q, raw[:1], CAM)
        d_raw = torch.from_numpy(np.ascontiguousarray(raw[1:])).cuda()
        bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, P)]
        d_m = torch.zeros(2 * 12, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ptr = [b.data_ptr() + GUARD for b in bufs]
        ps = np.ascontiguousarray(poses[1:], np.float64)
        ids = np.array([0, 0], np.int32)

        def call(n_=n, ids_=ids, ps_=ps, raw_=d_raw.data_ptr(), cam_=cam, m_=None, stride=12, out=tuple(ptr), mem=api.SN_MEM_DEVICE):
            return lib.sn_elevation_push(ev._e, n_, None if ids_ is None else ids_.ctypes.data, ps_.ctypes.data if ps_ is not None else None,
                                         raw_, C.byref(cam_) if cam_ is not None else None, m_, stride, *[o or None for o in out], None, mem, None)

        bad_pose, far_pose = ps.copy(), ps.copy()
        bad_pose[1, 2], far_pose[0, 0] = np.nan, 2.0 ** 30 / el.units(P).k256 * 1.01
        step3, nofx = api._sn_camera(dataclasses.replace(CAM, step=3), W, H), api._sn_camera(dataclasses.replace(CAM, fx=0.0), W, H)
        refused = {
            "n = 0": dict(n_=0), "n > max_batch": dict(n_=MAX_BATCH + 1), "no poses": dict(ps_=None), "no raw": dict(raw_=None),
            "no camera": dict(cam_=None), "step 3": dict(cam_=step3), "fx 0": dict(cam_=nofx), "a NaN pose": dict(ps_=bad_pose),
            "a pose too far": dict(ps_=far_pose), "a stream id of 2": dict(ids_=np.array([0, 2], np.int32)),
            "a stream id of -1": dict(ids_=np.array([-1, 0], np.int32)), "no output": dict(out=(0, 0, 0, 0, 0)),
            "hi misaligned": dict(out=(ptr[0], ptr[1] + 1, ptr[2], ptr[3], ptr[4])), "rise misaligned": dict(out=(ptr[0], ptr[1], ptr[2], ptr[3] + 1, ptr[4])),
            "stats misaligned": dict(out=(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4] + 2)), "raw misaligned": dict(raw_=d_raw.data_ptr() + 2),
            "mounts misaligned": dict(m_=d_m.data_ptr() + 2), "mount_stride 11": dict(m_=d_m.data_ptr(), stride=11),
            "trav over hi": dict(out=(ptr[1] + 4, ptr[1], ptr[2], ptr[3], ptr[4])), "lo over rise": dict(out=(ptr[0], ptr[1], ptr[3] + 8, ptr[3], ptr[4])),
            "raw is an output": dict(out=(ptr[0], d_raw.data_ptr(), ptr[2], ptr[3], ptr[4])),
            "mounts are an output": dict(m_=d_m.data_ptr(), out=(ptr[0], ptr[1], ptr[2], ptr[3], d_m.data_ptr() + 16)),
            "a bad mem": dict(mem=7),
        }
        for why, kw in refused.items():
            assert call(**kw) == ERR_ARG, why
            assert lib.sn_last_error(eng._h).decode().startswith("sn_elevation_push: "), why
        assert lib.sn_elevation_reset(ev._e, 2) == ERR_ARG and lib.sn_elevation_reset(ev._e, -2) == ERR_ARG
        torch.cuda.synchronize()
        for name, b in zip(NAMES, bufs):
            assert bool((b == 0x5a).all()), f"a refused call wrote {name}"
        assert torch.equal(d_raw.cpu(), torch.from_numpy(np.ascontiguousarray(raw[1:]))) and not bool(d_m.any())
        # the state is where the first frame left it: both streams go on as the twin's
        ids2 = [0, 1]
        got, q2 = _device(torch, ev, P, poses[1:], raw[1:], CAM, ids=ids2)
        assert not _differing(got, twin.push(q2, raw[1:], CAM, stream_of=ids2))
    bad = [dict(mw=0), dict(mh=4097), dict(cell_m=0.0), dict(z_min_m=-33.0), dict(z_min_m=1.0, z_max_m=0.0), dict(range_max_m=0.0), dict(min_points=0),
           dict(alpha=0), dict(alpha=257), dict(max_step_mm=0), dict(max_step_mm=32768), dict(radius=0), dict(radius=4), dict(flags=1),
           dict(base_from_cam=(float("nan"),) + (0.0,) * 11), dict(cell_m=float("inf"))]
    for kw in bad:
        p = dataclasses.replace(P, **kw)
        assert el.check(p), kw
        with pytest.raises(api.StereoNetError):
            eng.elevation(p)
    for streams in (0, MAX_BATCH + 1):
        with pytest.raises(api.StereoNetError):
            eng.elevation(P, streams=streams)


@pytest.mark.gpu
def test_sn_destroy_is_refused_while_an_elevation_map_lives(model_factory):
    e = api.StereoNetHIP(model_factory(W, H, D), max_batch=1)
    ev = e.elevation(P)
    assert e._lib.sn_destroy(e._h) == ERR_BUSY and "elevation" in e._lib.sn_last_error(e._h).decode()
    ev.close()
    e.close()
    # a host-only object serves pose_q alone
    lib, obj = api.load_library(), C.c_void_p()
    prm = api.elevation_params(P)
    assert lib.sn_elevation_create(None, 5, C.byref(prm), C.byref(obj)) == 0
    q, pose = np.zeros(6, np.int32), np.array([0.35, -0.45, 0.5])
    assert lib.sn_elevation_pose_q(obj, pose.ctypes.data, q.ctypes.data) == 0 and q.tolist()[:2] == [448, -576] and q.tolist()[4:] == [1 - 35, -3 - 16]
    assert np.abs(q - el.pose_q(P, pose)).max() <= 1
    assert lib.sn_elevation_push(obj, 1, None, pose.ctypes.data, None, None, None, 12, None, None, None, None, None, None, 0, None) == ERR_ARG
    lib.sn_elevation_destroy(obj)
