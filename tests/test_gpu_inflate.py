"""sn_inflate_grid on the MI355X: cost, grid, dist2 and stats equal the numpy twin's (hobot_stereonet_amd/inflate.py) byte for
byte, the twin fed the library's table, with 16 guard bytes of 0x5a on either side of every wanted output and cost / grid at an
odd address: grids of one cell, one column, one row, a tile less one, a tile, a tile plus one, several tiles with tails, and a
strip wider than four tiles, each at R = 0, 1, 3, 16 (and 64 on 65 x 17, 130 x 33 and a grid of five tile rows), in both forms
of the kernel (SN_INFLATE_WAVES) and in a call large enough for the form to change by itself, with
obstacles at the corners, on both sides of the tile seams, exactly R and R^2 + 1 away across a seam, in equidistant pairs, tiles
away from the cells they reach, everywhere, nowhere, and in one map of a batch only; every subset of the outputs, both flag
values, lethal_min 100 and 65, host mode and device mode on a caller stream; two parameter blocks alternating on one handle;
beside inference; ground -> obstacles -> costmap -> inflate on one stream from the engine's own map; argument errors; the node's
topic and the filelist tool.

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

from hobot_stereonet_amd import api, costmap, ground, inflate, obstacles, synth, weights
from hobot_stereonet_amd.costmap import CostmapParams
from hobot_stereonet_amd.ground import GroundParams
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG = -1      # SN_ERR_ARG (include/stereonet_hip.h)
NAMES = ("cost", "grid", "dist2", "stats")
DTYPES = (np.uint8, np.int8, np.uint16, np.uint32)
OFFSET = (GUARD + 1, GUARD + 1, GUARD, GUARD)      # cost and grid at an odd address
ALL = (True, True, True, True)
TW, TH = 64, 16      # the kernel's tile


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _forced(model_factory, waves):
    """an engine created under SN_INFLATE_WAVES (read by sn_create): that form of the kernel whatever the call's size"""
    before = os.environ.get("SN_INFLATE_WAVES")
    os.environ["SN_INFLATE_WAVES"] = str(waves)
    try:
        return api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH)
    finally:
        if before is None:
            del os.environ["SN_INFLATE_WAVES"]
        else:
            os.environ["SN_INFLATE_WAVES"] = before


@pytest.fixture(scope="module")
def engines(eng, model_factory):
    """by size (these tests' calls are small: the wide form), and each form forced"""
    with _forced(model_factory, 4) as e4, _forced(model_factory, 16) as e16:
        yield {"by size": eng, "4 waves": e4, "16 waves": e16}


def _params(R, **kw):
    """cell 0.125 m and radii that are multiples of it: R exactly; the inscribed radius covers d2 = 1 and 2, the fall-off the rest"""
    return InflateParams(**dict(dict(cell_m=0.125, inscribed_radius_m=min(0.18, 0.125 * R), inflation_radius_m=0.125 * R, cost_scaling=0.9,
                                     lethal_min=100, flags=0), **kw))


def _sizes(n, gw, gh):
    return (n * gw * gh, n * gw * gh, 2 * n * gw * gh, 20 * n)


def _shaped(n, gw, gh, parts):
    shapes = ((n, gh, gw), (n, gh, gw), (n, gh, gw), (n, 5))
    return [None if b is None else b.view(d).reshape(s) for b, d, s in zip(parts, DTYPES, shapes)]


def _device(torch, eng, occ, p, want=ALL, stream=0):
    """device mode: occ uploaded, every wanted output between GUARD bytes of 0x5a in a buffer of its own (cost and grid at an
    odd address) -> the four outputs (None where not wanted), after checking every byte the call must not write"""
    n, gh, gw = occ.shape
    d_occ = torch.from_numpy(np.array(occ)).cuda()
    sizes = _sizes(n, gw, gh)
    bufs = [torch.full((s + off + GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, off, w_ in zip(sizes, OFFSET, want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + off if b is not None else 0 for b, off in zip(bufs, OFFSET)]
    assert all(b is None or b.data_ptr() % 4 == 0 for b in bufs)
    eng.inflate_device(n, d_occ.data_ptr(), gw, gh, p, *ptrs, stream=stream)
    if stream:
        torch.cuda.synchronize()
    parts = []
    for name, b, s, off in zip(NAMES, bufs, sizes, OFFSET):
        if b is None:
            parts.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[:off] == 0x5a) and np.all(o[off + s:] == 0x5a), f"guard bytes around {name}"
        parts.append(o[off:off + s].copy())
    return _shaped(n, gw, gh, parts)


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


def _placed(gw, gh, R, seed):
    """eight maps of one geometry -> (occ int8 (8, gh, gw), what each map is)"""
    rng = np.random.default_rng(seed)
    occ = rng.choice(np.array([-1, 0, 40, 99], np.int8), (8, gh, gw), p=(0.35, 0.45, 0.1, 0.1))
    sx, sy = min(TW - 1, gw - 1), min(TH - 1, gh - 1)      # the last column / row of the first tile
    what = []
    occ[0, [0, 0, gh - 1, gh - 1], [0, gw - 1, 0, gw - 1]] = 100
    what.append("the four corners")
    for x, y in ((sx, 0), (min(sx + 1, gw - 1), gh - 1), (0, sy), (gw - 1, min(sy + 1, gh - 1)), (sx, sy), (min(sx + 1, gw - 1), min(sy + 1, gh - 1))):
        occ[1, y, x] = 100
    what.append("both sides of the seams x = 63 | 64 and y = 15 | 16")
    occ[2, sy, sx] = 100
    what.append("one obstacle in the corner of the first tile: cells exactly R and R^2 + 1 away lie across both seams")
    k = max(1, min(R, (gw - 1) // 2))
    occ[3, gh // 2, max(0, gw // 2 - k)] = 100
    occ[3, gh // 2, min(gw - 1, gw // 2 - k + 2 * k)] = 100
    occ[3, 0, gw // 2] = 100
    occ[3, min(gh - 1, 2 * (gh // 2)), gw // 2] = 100
    what.append("pairs of obstacles with cells at the same distance from both")
    occ[4, 0, 0] = 100
    what.append("one obstacle at the origin: the cells it reaches lie tiles away")
    occ[5] = 100
    what.append("every cell an obstacle")
    what.append("no obstacle (the skip path)")
    occ[7] = -1
    what.append("every cell unknown")
    return occ, what


GEOMETRIES = [(1, 1), (1, 40), (40, 1), (63, 15), (64, 16), (65, 17), (130, 33), (257, 3)]


def _radii(gw, gh):
    return (0, 1, 3, 16) + ((64,) if (gw, gh) in ((65, 17), (130, 33), (70, 70)) else ())


@pytest.mark.gpu
@pytest.mark.parametrize("gw,gh", GEOMETRIES + [(70, 70)])
def test_geometries_radii_and_placements(engines, gw, gh):
    """(70, 70) is five tile rows: at R = 64 the nearest obstacle of a cell lies up to four tile rows away.  Every case in
    both forms of the kernel."""
    import torch
    for R in _radii(gw, gh):
        for flags in ((0, 1) if R in (3, 64) else (R & 1,)):
            p = _params(R, flags=flags)
            assert inflate.radius_cells(p) == R
            occ, what = _placed(gw, gh, R, seed=gw * 131 + gh * 7 + R)
            T = api.inflate_table(p)
            want = inflate.reference(occ, p, T)
            for form, e in engines.items():
                got = _device(torch, e, occ, p)
                bad = _differing(got, want)
                if bad:
                    first = [what[k] for k in range(8) if any(g[k].tobytes() != w_[k].tobytes() for g, w_ in zip(got, want))]
                    raise AssertionError((form, gw, gh, R, flags, bad, first, got[3].tolist(), want[3].tolist()))
                assert np.array_equal(got[3].sum(1), [gw * gh] * 8)
            sx, sy = min(TW - 1, gw - 1), min(TH - 1, gh - 1)
            if R > 0 and ((gh > 1 and (sx >= R or sx + R < gw)) or (gw > 1 and (sy >= R or sy + R < gh))):
                one = inflate.reference(occ[2], p, T)[4]      # the grid holds cells (R, 0) and (R, 1) away from map 2's one obstacle
                assert one["at_r2"] > 0 and one["past_r2"] > 0 and one["obstacle"] == 1, (gw, gh, R, one)


@pytest.mark.gpu
def test_a_call_of_more_workgroups_than_are_resident_at_once(engines):
    """by size, a call takes the 4-wave form once it has more workgroups than two per CU: 8 maps of 520 x 130 are 8 x 81"""
    import torch
    gw, gh, n = 520, 130, 8
    tiles = -(-gw // TW) * -(-gh // TH)
    assert tiles * n > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(77)
    occ = rng.choice(np.array([-1, 0, 99, 100], np.int8), (n, gh, gw), p=(0.3, 0.68, 0.0197, 0.0003))
    occ[3], occ[5, :, :200] = 0, -1
    for R in (3, 16):
        p = _params(R, flags=R & 1)
        want = inflate.reference(occ, p, api.inflate_table(p))
        assert want[4]["at_r2"] > 0 and want[4]["past_r2"] > 0 and want[3][3].tolist() == [0, 0, 0, gw * gh, 0]
        for form, e in engines.items():
            assert not _differing(_device(torch, e, occ, p), want), (form, R)


@pytest.mark.gpu
def test_the_nearest_obstacle_three_and_more_tiles_away(eng):
    """R = 64 on 130 x 33 and 70 x 70: obstacles in the first tile row alone, so the cells of the third (and, at 70 x 70, fourth
    and fifth) tile row find their nearest obstacle two to four seams away, some at d2 = R^2 exactly"""
    import torch
    p = _params(64, flags=1)
    for gw, gh in ((130, 33), (70, 70)):
        occ = np.zeros((2, gh, gw), np.int8)
        occ[0, 0, 5], occ[0, 3, gw - 2] = 100, 100
        occ[1, :, ::2] = -1
        occ[1, 0, gw // 2] = 100
        want = inflate.reference(occ, p, api.inflate_table(p))
        far = want[2][:, 2 * TH:][want[2][:, 2 * TH:] != inflate.NOT_REACHED]
        assert far.size > 0 and (gh < 65 or (want[2][1, 64, gw // 2] == 4096 and want[2][1, 65, gw // 2] == inflate.NOT_REACHED))
        assert not _differing(_device(torch, eng, occ, p), want), (gw, gh)


@pytest.mark.gpu
def test_one_map_of_a_batch_with_obstacles(eng):
    import torch
    p = _params(16)
    occ, _ = _placed(130, 33, 16, seed=5)
    batch = np.stack([occ[6], occ[7], occ[1], occ[6], occ[7]])
    want = inflate.reference(batch, p, api.inflate_table(p))
    assert want[4]["obstacle"] == 6 and np.all(want[3][[0, 1, 3, 4], :3] == 0) and want[3][2, 0] == 6
    assert not _differing(_device(torch, eng, batch, p), want)


@functools.lru_cache(maxsize=None)
def _boundary(flags=0, lethal_min=65):
    """inflate.boundary_scene with the library's table, and the twin's answer to it: shared by the tests and never changed"""
    p, occ = inflate.boundary_scene()
    p = dataclasses.replace(p, flags=flags, lethal_min=lethal_min)
    want = inflate.reference(occ, p, api.inflate_table(p))
    for a in (occ,) + want[:4]:
        a.setflags(write=False)
    return p, occ, want


@pytest.mark.gpu
def test_every_subset_of_the_outputs_flags_and_lethal_min_in_both_memory_modes(eng):
    import torch
    side = torch.cuda.Stream()
    for flags, lethal_min in ((0, 65), (1, 65), (0, 100), (1, 100)):
        p, occ, want = _boundary(flags, lethal_min)
        for sub in itertools.product((False, True), repeat=4):
            if not any(sub):
                continue
            for stream in (0, side.cuda_stream):                               # blocking | a caller stream
                assert not _differing(_device(torch, eng, occ, p, want=sub, stream=stream), want), (flags, lethal_min, sub, stream)
            got = eng.inflate(occ, p, want=sub)                                # host mode
            assert [g is not None for g in got] == list(sub) and not _differing(got, want), (flags, lethal_min, sub)
    # lethal_min moves the obstacles, the flag the unknown cells of the fall-off
    a, b, c = _boundary(0, 65)[2], _boundary(0, 100)[2], _boundary(1, 65)[2]
    assert a[4]["obstacle"] > b[4]["obstacle"] > 0 and a[0].tobytes() != c[0].tobytes()
    one = eng.inflate(_boundary()[1][0], _boundary()[0])                       # a 2-D grid in, 2-D maps out
    assert one[0].shape == (21, 37) and one[3].shape == (5,) and np.array_equal(one[0], a[0][0])


@pytest.mark.gpu
def test_two_parameter_blocks_alternating_on_one_handle(eng):
    """the lane keeps the last block's table on the device: a call with another block must not see it"""
    import torch
    side = torch.cuda.Stream()
    p1, occ, want1 = _boundary()
    p2 = _params(7, cost_scaling=0.4, lethal_min=64, flags=1)
    p3 = dataclasses.replace(p1, cost_scaling=0.5)                             # the same R, another table
    want2, want3 = inflate.reference(occ, p2, api.inflate_table(p2)), inflate.reference(occ, p3, api.inflate_table(p3))
    assert want1[0].tobytes() != want3[0].tobytes()
    for stream in (side.cuda_stream, 0):
        for _ in range(2):
            for p, want in ((p1, want1), (p2, want2), (p3, want3), (p3, want3)):
                assert not _differing(_device(torch, eng, occ, p, stream=stream), want), (p, stream)


@pytest.mark.gpu
def test_inflate_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread inflates (ctypes drops the GIL): the maps of both equal the serial run's."""
    p, occ, want = _boundary()
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=MAX_BATCH) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, rounds = [], []

        def work():
            try:
                for _ in range(12):
                    if _differing(e.inflate(occ, p), want):
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


def _inflation_for(op, lethal_min):
    """a robot of 1.2 cells inside 3 cells of inflation on the obstacle grid's cell"""
    return InflateParams(cell_m=op.cell_m, inscribed_radius_m=float(np.float32(1.2 * op.cell_m)), inflation_radius_m=float(np.float32(3 * op.cell_m)),
                         cost_scaling=float(np.float32(0.5 / op.cell_m)), lethal_min=lethal_min, flags=inflate.UNKNOWN)


@pytest.mark.gpu
def test_end_to_end_on_the_device_from_the_engines_own_map(eng):
    """sn_infer_batch -> sn_ground_from_raw -> sn_obstacles_from_raw_mounts -> sn_costmap_push -> sn_inflate_grid on one stream:
    nothing crosses to the host in between; the obstacle grid is inflated too"""
    import torch
    n = 4
    x = np.stack([synth.model_input_i8(W, H, D, 20 + k) for k in range(n)])
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    raw_host = np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)])
    gp, op, p = _scene_params(raw_host, cam, True, eng.out_scale)
    ip_map, ip_occ = _inflation_for(op, 65), _inflation_for(op, 100)
    poses = np.array([[0.0, 0.0, 0.0], [op.cell_m * 1.5, 0.0, 0.1], [op.cell_m * 3.0, op.cell_m, 0.2], [op.cell_m * 3.0, -op.cell_m, -0.4]])
    d_in = torch.from_numpy(x).cuda()
    d_raw = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    d_rec = torch.zeros(n * ground.RECORD.itemsize, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n * op.gw * op.gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_rng = torch.full((n * op.beams,), 7.0, dtype=torch.float32, device="cuda")
    d_map = torch.full((n * p.mw * p.mh,), 0x5a, dtype=torch.uint8, device="cuda")
    outs_map = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, p.mw, p.mh)]
    outs_occ = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, op.gw, op.gh)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with eng.costmap(op, p) as cm:
        eng.infer_device(n, d_in.data_ptr(), d_raw.data_ptr(), 0, stream=st.cuda_stream)
        eng.ground_device(n, d_raw.data_ptr(), cam, gp, d_rec.data_ptr(), 0, stream=st.cuda_stream)
        eng.obstacles_device(n, d_raw.data_ptr(), cam, op, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr(), stream=st.cuda_stream,
                             mounts_ptr=d_rec.data_ptr() + 4 * ground.MOUNT_OFFSET_FLOATS, mount_stride=ground.RECORD_FLOATS)
        q = cm.push_device(n, poses, d_occ.data_ptr(), d_rng.data_ptr(), None, d_map.data_ptr(), 0, 0, stream=st.cuda_stream)
        eng.inflate_device(n, d_map.data_ptr(), p.mw, p.mh, ip_map, *[o.data_ptr() for o in outs_map], stream=st.cuda_stream)
        eng.inflate_device(n, d_occ.data_ptr(), op.gw, op.gh, ip_occ, *[o.data_ptr() for o in outs_occ], stream=st.cuda_stream)
        torch.cuda.synchronize()
    raw = d_raw.cpu().numpy()
    assert np.array_equal(raw, raw_host)
    # the twins of the four stages, each fed what the chain says it is fed
    rec = ground.reference(raw, cam, gp, gate_q16=api.ground_gate(cam, gp, W, H), labels=False, out_scale=eng.out_scale)[0]
    edges = api.beam_edges(op)
    ref = [obstacles.reference(raw[k], cam, dataclasses.replace(op, base_from_cam=tuple(rec["base_from_cam"][k])), edges=edges,
                               out_scale=eng.out_scale) for k in range(n)]
    occ, rng = np.stack([r[0] for r in ref]), np.stack([r[3] for r in ref])
    assert d_occ.cpu().numpy().view(np.int8).tobytes() == occ.tobytes()
    grid = costmap.Reference(p, op, edges=edges).push(q, occ, rng)[0]
    assert d_map.cpu().numpy().view(np.int8).tobytes() == grid.tobytes()
    want_map = inflate.reference(grid, ip_map, api.inflate_table(ip_map))
    want_occ = inflate.reference(occ, ip_occ, api.inflate_table(ip_occ))
    print("end to end stats:", want_map[3].tolist(), want_occ[3].tolist())
    assert want_map[4]["obstacle"] > 0 and want_map[4]["decayed"] > 0 and want_occ[4]["obstacle"] > 0      # a scene, not an empty map
    assert not _differing(_shaped(n, p.mw, p.mh, [o.cpu().numpy() for o in outs_map]), want_map)
    assert not _differing(_shaped(n, op.gw, op.gh, [o.cpu().numpy() for o in outs_occ]), want_occ)


@pytest.mark.gpu
def test_argument_errors_change_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    p, occ, want = _boundary()
    n, gh, gw = occ.shape
    c_p = api.inflate_params(p)
    sizes = _sizes(MAX_BATCH, gw, gh)
    d_occ = torch.from_numpy(occ.copy()).cuda()
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [b.data_ptr() + GUARD for b in bufs]
    torch.cuda.synchronize()

    def failed(rc):
        msg = lib.sn_last_error(hnd).decode()
        return rc == ERR_ARG and msg.startswith("sn_inflate_grid: ") and len(msg) > len("sn_inflate_grid: ")

    def call(n=n, o=None, gw=gw, gh=gh, prm=c_p, out=None, mem=api.SN_MEM_DEVICE, h=hnd):
        out = ptr if out is None else out
        return lib.sn_inflate_grid(h, n, (d_occ.data_ptr() if o is None else o) or None, gw, gh, None if prm is None else C.byref(prm),
                                   *[v or None for v in out], mem, None)

    bad_p = {k: api.inflate_params(dataclasses.replace(p, **kw)) for k, kw in
             {"cell 0": dict(cell_m=0.0), "cell nan": dict(cell_m=math.nan), "inscribed < 0": dict(inscribed_radius_m=-1.0),
              "inflation < inscribed": dict(inflation_radius_m=0.1), "inflation inf": dict(inflation_radius_m=math.inf),
              "scaling < 0": dict(cost_scaling=-0.5), "scaling nan": dict(cost_scaling=math.nan), "R = 65": dict(inflation_radius_m=16.26),
              "flags 2": dict(flags=2), "flags 5": dict(flags=5), "lethal_min 0": dict(lethal_min=0), "lethal_min 101": dict(lethal_min=101)}.items()}
    bad = {"n = 0": dict(n=0), "n < 0": dict(n=-3), "n > max_batch": dict(n=MAX_BATCH + 1), "null occ": dict(o=0), "null params": dict(prm=None),
           "gw 0": dict(gw=0), "gh 0": dict(gh=0), "gw 4097": dict(gw=4097), "gh 4097": dict(gh=4097), "gw < 0": dict(gw=-1),
           "bad mem": dict(mem=7), "no outputs": dict(out=[0, 0, 0, 0]),
           "dist2 odd": dict(out=[ptr[0], ptr[1], ptr[2] + 1, ptr[3]]), "stats misaligned": dict(out=[ptr[0], ptr[1], ptr[2], ptr[3] + 2]),
           "cost is occ": dict(out=[d_occ.data_ptr(), 0, 0, 0]), "grid is occ": dict(out=[0, d_occ.data_ptr(), 0, 0]),
           "grid overlaps the end of occ": dict(out=[ptr[0], d_occ.data_ptr() + n * gw * gh - 1, ptr[2], ptr[3]]),
           "dist2 overlaps occ": dict(out=[ptr[0], ptr[1], d_occ.data_ptr() + 8, ptr[3]]),
           "stats overlaps occ": dict(out=[ptr[0], ptr[1], ptr[2], d_occ.data_ptr() + 4]),
           "cost overlaps grid": dict(out=[ptr[1] + 5, ptr[1], ptr[2], ptr[3]]), "cost overlaps dist2": dict(out=[ptr[2] + 2 * n * gw * gh - 1, ptr[1], ptr[2], ptr[3]]),
           "grid overlaps stats": dict(out=[ptr[0], ptr[3] + 3, ptr[2], ptr[3]]), "dist2 overlaps stats": dict(out=[ptr[0], ptr[1], ptr[3] + 4, ptr[3]])}
    bad.update({k: dict(prm=v) for k, v in bad_p.items()})
    for name, kw in bad.items():
        assert failed(call(**kw)), name
    assert call(h=None) == ERR_ARG
    with pytest.raises(api.StereoNetError):
        eng.inflate(occ[0, 0], p)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5a).all()) for b in bufs), "a refused call wrote something"
    # the bounds themselves are allowed, and the first good call after all that is right
    assert call(n=1, gw=gw * gh, gh=1, out=[ptr[0], 0, 0, 0]) == 0 and call(n=1, gw=1, gh=gw * gh, out=[ptr[0], 0, 0, 0]) == 0
    assert call() == 0
    torch.cuda.synchronize()
    parts = []
    for b, s in zip(bufs, _sizes(n, gw, gh)):
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a)
        parts.append(o[GUARD:GUARD + s].copy())
    assert not _differing(_shaped(n, gw, gh, parts), want)


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    args = [os.path.join(COMPAT, "build", "inflate_harness"), model, frames, str(W), str(H), str(nframes), prefix]
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    msgs = {kind: [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith(kind + " ")] for kind in ("grid", "costmap", "inflated")}
    order = [l.split()[0] for l in lines if l.split()[0] in ("grid", "scan", "costmap", "inflated")]
    return msgs, order, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_inflated_grid(weights_blob, tmp_path):
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
        _, op, p = _scene_params(e.infer_sbs_nv12(sbs)[1].reshape(1, H, W), cam)
    op = dataclasses.replace(op, frame="base_footprint")
    p = dataclasses.replace(p, frame="map")
    ip = _inflation_for(op, 65)
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), p)
    inflate.save_params(str(tmp_path / "in.txt"), dataclasses.replace(ip, cell_m=123.0))      # the node takes the grid's cell, not the file's
    T = api.inflate_table(ip)
    cam_env = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0", "STEREONET_OBSTACLES": str(tmp_path / "ob.txt")}
    f_bin = str(tmp_path / "f.bin")
    msgs, order, _ = _run_harness(tmp_path, "off", m, f_bin, nframes, cam_env)
    assert not msgs["inflated"] and order == ["grid", "scan"] * nframes          # unset: nothing on the topic
    both = dict(cam_env, STEREONET_COSTMAP=str(tmp_path / "cm.txt"), STEREONET_INFLATE=str(tmp_path / "in.txt"))
    for tag, env, src, suffix, per_frame in (("chain", both, "costmap", "costmap", ["grid", "scan", "costmap", "inflated"]),
                                             ("grid", {k: v for k, v in both.items() if k != "STEREONET_COSTMAP"}, "grid", "grid",
                                              ["grid", "inflated", "scan"])):
        msgs, order, log = _run_harness(tmp_path, tag, m, f_bin, nframes, env)
        assert len(msgs["inflated"]) == nframes and order == per_frame * nframes and "/stereonet_inflated_grid" in log, (tag, order)
        for k in range(nframes):
            got, source = msgs["inflated"][k], msgs[src][k]
            for key in ("frame_id", "stamp", "width", "height", "resolution", "origin", "len"):      # info copied from its source
                assert got[key] == source[key], (tag, k, key)
            gw, gh = int(got["width"]), int(got["height"])
            data = np.fromfile(str(tmp_path / f"{tag}.{k}.{suffix}"), np.int8).reshape(1, gh, gw)
            want = inflate.reference(data, ip, T)
            assert open(tmp_path / f"{tag}.{k}.inflated", "rb").read() == want[1].tobytes(), (tag, k)
        assert want[4]["obstacle"] > 0
    # without the obstacle grid, or with a file the stage refuses, the node is as it is without the variable
    env = {k: v for k, v in cam_env.items() if k != "STEREONET_OBSTACLES"}
    msgs, order, log = _run_harness(tmp_path, "alone", m, f_bin, nframes, dict(env, STEREONET_INFLATE=str(tmp_path / "in.txt")))
    assert not msgs["inflated"] and not order and log.count("requires STEREONET_OBSTACLES") == 1 and log.count("no inflated grid") == 1
    inflate.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(ip, lethal_min=0))
    msgs, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, dict(cam_env, STEREONET_INFLATE=str(tmp_path / "bad.txt")))
    assert not msgs["inflated"] and order == ["grid", "scan"] * nframes and log.count("no inflated grid") == 1


@pytest.mark.gpu
def test_filelist_writes_the_inflated_grid(model_factory, tmp_path, capsys):
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
    ip = _inflation_for(op, 65)
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), p)
    inflate.save_params(str(tmp_path / "in.txt"), dataclasses.replace(ip, cell_m=9.0))      # the tool takes the obstacle file's cell
    T = api.inflate_table(ip)
    common = ["--model", model, "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120"]
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--inflate", str(tmp_path / "in.txt")])      # requires --obstacles
    inflate.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(ip, flags=4))
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--obstacles", str(tmp_path / "ob.txt"), "--inflate", str(tmp_path / "bad.txt")])
    capsys.readouterr()
    edges = api.beam_edges(op)
    for tag, extra in (("chain", ["--costmap", str(tmp_path / "cm.txt")]), ("grid", [])):
        out = str(tmp_path / tag)
        assert filelist.main(common + ["--out", out, "--obstacles", str(tmp_path / "ob.txt"), "--inflate", str(tmp_path / "in.txt")] + extra) == 0
        summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        twin = costmap.Reference(p, op, edges=edges)
        q = api.costmap_pose_q(p, op, np.zeros((n, 3)))
        for i in range(n):
            raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)
            occ, _, _, ranges, _ = obstacles.reference(raw, cam, op, edges=edges)
            src = twin.push(q[i:i + 1], occ[None], ranges[None])[0] if extra else occ[None]
            cost, _, _, stats, br = inflate.reference(src, ip, T)
            pgm = open(os.path.join(out, f"{i}.inflated.pgm"), "rb").read()
            assert pgm == f"P5\n{src.shape[2]} {src.shape[1]}\n255\n".encode() + cost[0].tobytes(), (tag, i)
            assert [summary["inflate"][k][i] for k in inflate.STATS] == stats[0].tolist() and sum(stats[0]) == src[0].size
        assert br["obstacle"] > 0 and summary["frames"] == n
