"""sn_navfn on the MI355X: potential, path and stats equal the heapq twin's (hobot_stereonet_amd/navfn.py) byte for byte, with 16
guard bytes of 0x5a on either side of every wanted output and cost at an odd address: grids of one cell, one row, one column, a
tile less one, a tile, a tile plus one, several tiles with tails and a strip wider than four tiles; empty, random, walled,
pinched, serpentine, closed and unknown cost fields; goals at the corners, on a seam, blocked and outside; every subset of the
outputs, host mode and device mode on a caller stream, a path one cell short, fixed rounds; inflate -> navfn on one stream from
the engine's own map; beside inference; argument errors; the node's topic and the filelist tool.

No tolerance appears: the contract is the same bytes.  (rounds_out depends on the schedule and is compared with nothing.)"""
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

from hobot_stereonet_amd import api, inflate, navfn, obstacles, synth, weights
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.navfn import INF, NavParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG = -1      # SN_ERR_ARG (include/stereonet_hip.h)
NAMES = ("potential", "path", "stats")
ALL = (True, True, True)
TW, TH = navfn.TILE_W, navfn.TILE_H      # the kernel's tile
P0 = NavParams(neutral=50, lethal_cost=253, unknown_cost=30, flags=0, max_rounds=0, max_path=700)


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _sizes(n, gw, gh, p):
    return (4 * n * gw * gh, 8 * n * p.max_path, 20 * n)


def _expected(want, p):
    """the twin's outputs as the bytes the call must leave in 0x5a-filled buffers: path entries past the length are not written"""
    pot, path, stats = want
    out = [pot.tobytes(), None, stats.tobytes()]
    if path is not None:
        raw = np.full(path.shape, 0x5a5a5a5a, np.int32)
        for k in range(path.shape[0]):
            m = min(int(stats[k, 2]), p.max_path)
            raw[k, :m] = path[k, :m]
        out[1] = raw.tobytes()
    return out


def _device(torch, eng, cost, goals, starts, p, want=ALL, stream=0):
    """device mode: cost uploaded to an odd address, goals and starts uploaded, every wanted output between GUARD bytes of 0x5a in
    a buffer of its own -> (the three outputs as bytes, None where not wanted; rounds), after checking the guards"""
    n, gh, gw = cost.shape
    d_cost = torch.zeros(cost.size + 1, dtype=torch.uint8, device="cuda")
    d_cost[1:] = torch.from_numpy(np.array(cost).reshape(-1)).cuda()
    d_goals = torch.from_numpy(np.array(goals, np.int32)).cuda()
    d_starts = None if starts is None else torch.from_numpy(np.array(starts, np.int32)).cuda()
    sizes = _sizes(n, gw, gh, p)
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(sizes, want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
    assert d_cost.data_ptr() % 2 == 0
    rounds = eng.navfn_device(n, d_cost.data_ptr() + 1, gw, gh, d_goals.data_ptr(), 0 if d_starts is None else d_starts.data_ptr(), p,
                              *ptrs, stream=stream)
    torch.cuda.synchronize()
    parts = []
    for name, b, s in zip(NAMES, bufs, sizes):
        if b is None:
            parts.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a), f"guard bytes around {name}"
        parts.append(o[GUARD:GUARD + s].tobytes())
    return parts, rounds


def _differing(got, want, p):
    """the names of the outputs whose bytes differ from the twin's"""
    return [name for name, g, w_ in zip(NAMES, got, _expected(want, p)) if g is not None and g != w_]


def _fields(gw, gh, seed):
    """eight cost fields of one geometry with a goal and a start each -> (cost uint8 (8, gh, gw), goals, starts, what each is)"""
    rng = np.random.default_rng(seed)
    cost = np.zeros((8, gh, gw), np.uint8)
    sx, sy = min(TW - 1, gw - 1), min(TH - 1, gh - 1)      # the last column / row of the first tile
    far = (gw - 1, gh - 1)
    goals, starts, what = [], [], []
    what.append("empty and uniform: every tie rule is live; goal in the far corner")
    goals.append(far), starts.append((0, 0))
    cost[1] = rng.integers(0, 253, (gh, gw))
    if (gw - 1, 0) != (sx, sy):
        cost[1, 0, gw - 1] = 254
    what.append("random 0..252; goal on the seam; a blocked start")
    goals.append((sx, sy)), starts.append((gw - 1, 0))
    if gw > 2 and gh > 1:
        cost[2, :, min(sx, gw - 2)] = 254
        cost[2, gh // 2, min(sx, gw - 2)] = 0
    what.append("a wall on the last column of the first tile with one gap; goal top right")
    goals.append((gw - 1, 0)), starts.append((0, gh - 1))
    if gw > sx + 1 and gh > sy + 1:
        cost[3, sy + 1, sx], cost[3, sy, sx + 1] = 254, 253      # the diagonal (sx, sy) - (sx + 1, sy + 1) is pinched across four tiles
    what.append("a diagonal pinch of two blocked cells at the first tile corner; goal just past it")
    goals.append((min(sx + 1, gw - 1), min(sy + 1, gh - 1))), starts.append((max(sx - 1, 0), max(sy - 1, 0)))
    cost[4] = rng.choice(np.array([0, 0, 0, 90, 252, 253, 254, 255], np.uint8), (gh, gw))
    cost[4, 0, 0] = 0
    what.append("random with lethal and unknown cells; goal at the origin")
    goals.append((0, 0)), starts.append(far)
    if gw >= 5 and gh >= 5:
        cost[5, gh // 2 - 2:gh // 2 + 3, gw // 2 - 2:gw // 2 + 3] = 254
        cost[5, gh // 2 - 1:gh // 2 + 2, gw // 2 - 1:gw // 2 + 2] = 0
    what.append("a closed room around the start; goal bottom left")
    goals.append((0, gh - 1)), starts.append((gw // 2, gh // 2))
    cost[6] = rng.choice(np.array([0, 40, 255], np.uint8), (gh, gw), p=(0.6, 0.2, 0.2))
    cost[6, gh - 1, gw - 1] = 254
    what.append("unknown cells; a blocked goal")
    goals.append(far), starts.append((0, 0))
    cost[7] = rng.integers(0, 200, (gh, gw))
    cost[7, 0, 0] = 254
    what.append("a goal outside the grid and a blocked start")
    goals.append((gw, 0)), starts.append((0, 0))
    return cost, np.array(goals, np.int32), np.array(starts, np.int32), what


GEOMETRIES = [(1, 1), (40, 1), (1, 40), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 6, TH + 13), (4 * TW + 22, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("gw,gh", GEOMETRIES)
def test_geometries_and_cost_fields(eng, gw, gh):
    import torch
    cost, goals, starts, what = _fields(gw, gh, seed=gw * 131 + gh * 7)
    for flags in (0, navfn.UNKNOWN_OK):
        p = dataclasses.replace(P0, flags=flags)
        want = navfn.reference(cost, goals, starts, p)
        got, rounds = _device(torch, eng, cost, goals, starts, p)
        bad = _differing(got, want, p)
        if bad:
            pot = np.frombuffer(got[0], np.uint32).reshape(want[0].shape)
            first = [what[k] for k in range(8) if pot[k].tobytes() != want[0][k].tobytes()]
            raise AssertionError((gw, gh, flags, bad, first, np.frombuffer(got[2], np.uint32).reshape(8, 5).tolist(), want[2].tolist()))
        assert rounds >= 1
        st = want[2]
        assert st[0, 0] == 0 and st[0, 2] == max(gw, gh) and np.all(st[:, 1] + st[:, 4] <= gw * gh)
        assert gw * gh == 1 or (st[1, 0] == navfn.START_UNREACHABLE and st[1, 1] == gw * gh - 1 and st[1, 4] == 1)
        assert st[6, 0] & navfn.GOAL_BLOCKED and st[7, 0] == navfn.GOAL_BLOCKED | navfn.START_UNREACHABLE and st[7, 1] == 0
        if gw >= 5 and gh >= 5:
            assert st[5, 0] == navfn.START_UNREACHABLE and st[5, 1] > 0
    if gw == 1 and gh == 1:      # goal = start: a path of one cell
        one = navfn.reference(cost[:1], [(0, 0)], [(0, 0)], P0)
        assert one[2][0].tolist() == [0, 1, 1, 0, 0]
        assert not _differing(_device(torch, eng, cost[:1], np.array([[0, 0]]), np.array([[0, 0]]), P0)[0], one, P0)


def _serpentine(gw, gh):
    """corridors on the even rows over the whole width, joined at alternating ends: the route crosses every vertical seam in
    every corridor and comes back through tiles that had settled -> cost uint8 (gh, gw)"""
    cost = np.full((gh, gw), 254, np.uint8)
    cost[0::2] = 0
    for i, y in enumerate(range(1, gh, 2)):
        cost[y, gw - 1 if i % 2 == 0 else 0] = 0
    return cost


@functools.lru_cache(maxsize=None)
def _winding():
    """a batch of three on 70 x 45 (3 x 2 tiles): the serpentine, an empty map, the serpentine again with another goal; and the
    twin's answer: shared by the tests and never changed"""
    gw, gh = 2 * TW + 6, TH + 13
    cost = np.stack([_serpentine(gw, gh), np.zeros((gh, gw), np.uint8), _serpentine(gw, gh)])
    goals = np.array([[0, 0], [gw - 1, gh - 1], [gw // 2, gh - 1]], np.int32)
    starts = np.array([[gw // 2, gh - 1], [0, 0], [3, 0]], np.int32)
    p = dataclasses.replace(P0, max_path=2000)
    want = navfn.reference(cost, goals, starts, p)
    for a in (cost, goals, starts) + want:
        a.setflags(write=False)
    return p, cost, goals, starts, want


@pytest.mark.gpu
def test_a_serpentine_needs_many_rounds_and_reactivates_settled_tiles(eng):
    import torch
    p, cost, goals, starts, want = _winding()
    gh, gw = cost.shape[1:]
    got, rounds = _device(torch, eng, cost, goals, starts, p)
    assert not _differing(got, want, p)
    corridors = (gh + 1) // 2
    assert want[2][0, 2] > corridors * (gw - 1) and rounds >= corridors      # a round per seam crossing at the very least
    print("serpentine rounds:", rounds)
    # obstacles in one map of the batch only, a different goal per map: map 1 is empty and equals its own single call
    alone = navfn.reference(cost[1:2], goals[1:2], starts[1:2], p)
    assert alone[0].tobytes() == want[0][1].tobytes() and want[2][1, 4] == 0 and want[2][0, 4] > 0
    assert not _differing(_device(torch, eng, cost[1:2], goals[1:2], starts[1:2], p)[0], alone, p)


@pytest.mark.gpu
def test_fixed_rounds(eng):
    import torch
    p, cost, goals, starts, want = _winding()
    side = torch.cuda.Stream()
    _, converged = _device(torch, eng, cost, goals, starts, p)
    # one round: the goal's tile alone has settled
    p1 = dataclasses.replace(p, max_rounds=1)
    got, rounds = _device(torch, eng, cost, goals, starts, p1)
    pot = np.frombuffer(got[0], np.uint32).reshape(want[0].shape)
    st = np.frombuffer(got[2], np.uint32).reshape(-1, 5)
    assert rounds == 1 and np.all(st[:, 0] & navfn.UNCONVERGED)
    assert np.all(pot >= want[0]) and np.any(pot > want[0]) and np.any((pot != INF) & (pot > 0))      # upper bounds, INF included
    assert np.array_equal(st[:, 4], want[2][:, 4]) and np.all(st[:, 1] < want[2][:, 1])
    # what the call made of its own unfinished field is what the twin makes of that field: the path ends, start unreachable or not
    again = navfn.reference(cost, goals, starts, p1, potential=pot)
    assert got[1] == _expected(again, p1)[1]
    assert np.array_equal(st[:, 1:], again[2][:, 1:]) and np.array_equal(st[:, 0], again[2][:, 0] | navfn.UNCONVERGED)
    # three rounds reach the start of the empty map (two tiles from its goal): whatever field the schedule left, the walk over it
    # ends at the goal and costs no more than the field says
    p3 = dataclasses.replace(p, max_rounds=3)
    got, _ = _device(torch, eng, cost, goals, starts, p3)
    pot = np.frombuffer(got[0], np.uint32).reshape(want[0].shape)
    st = np.frombuffer(got[2], np.uint32).reshape(-1, 5)
    again = navfn.reference(cost, goals, starts, p3, potential=pot)
    assert np.all(pot >= want[0]) and got[1] == _expected(again, p3)[1] and np.array_equal(st[:, 1:], again[2][:, 1:])
    assert st[1, 3] != INF and st[1, 2] >= max(cost.shape[1:]) and tuple(again[1][1, st[1, 2] - 1]) == tuple(goals[1])
    assert navfn.path_cost([tuple(c) for c in again[1][1, :st[1, 2]]], cost[1], p3) <= st[1, 3]
    # as many rounds as the converging call said did work, and one: the exact field, the flag clear; blocking and enqueued
    pr = dataclasses.replace(p, max_rounds=converged + 1)
    got, rounds = _device(torch, eng, cost, goals, starts, pr)
    assert not _differing(got, want, pr) and 1 <= rounds <= converged + 1
    got, rounds = _device(torch, eng, cost, goals, starts, pr, stream=side.cuda_stream)
    assert not _differing(got, want, pr) and rounds == -1                      # only enqueued: not known at return


@pytest.mark.gpu
def test_every_subset_of_the_outputs_in_both_memory_modes_and_a_short_path(eng):
    import torch
    side = torch.cuda.Stream()
    gw, gh = TW + 9, TH + 5
    cost, goals, starts, _ = _fields(gw, gh, seed=3)
    cost, goals, starts = cost[:5], goals[:5], starts[:5]
    for flags in (0, navfn.UNKNOWN_OK):
        p = dataclasses.replace(P0, flags=flags, max_path=100)
        want = navfn.reference(cost, goals, starts, p)
        assert not np.any(want[2][:, 0] & navfn.PATH_TRUNCATED)                 # that flag needs the path to be wanted
        for sub in itertools.product((False, True), repeat=3):
            if not any(sub):
                continue
            for stream in (0, side.cuda_stream):                                # the lane's stream | a caller stream
                assert not _differing(_device(torch, eng, cost, goals, starts, p, want=sub, stream=stream)[0], want, p), (flags, sub, stream)
            got = eng.navfn(cost, goals, starts, p, want=sub)                   # host mode
            assert [g is not None for g in got[:3]] == list(sub), sub
            for name, g, w_ in zip(NAMES, got[:3], want):
                assert g is None or (g.dtype == w_.dtype and g.tobytes() == w_.tobytes()), (flags, sub, name)
        # without starts: no path, no start flag, P(start) infinite
        none = navfn.reference(cost, goals, None, p)
        assert np.all(none[2][:, 2] == 0) and np.all(none[2][:, 3] == INF)
        got, _ = _device(torch, eng, cost, goals, None, p, want=(True, False, True))
        assert not _differing(got, none, p)
    # one cell short of the path: the truncation flag and the full length in the stats
    full = navfn.reference(cost, goals, starts, P0)[2]
    length = int(full[0, 2])
    assert length == max(gw, gh)
    short = dataclasses.replace(P0, max_path=length - 1)
    want = navfn.reference(cost, goals, starts, short)
    assert want[2][0, 0] == navfn.PATH_TRUNCATED and want[2][0, 2] == length
    assert not _differing(_device(torch, eng, cost, goals, starts, short)[0], want, short)
    # the same short max_path with the path not wanted: the flag is the flag of a path that was wanted, the length is still full
    unwanted = navfn.reference(cost, goals, starts, short, want_path=False)
    assert unwanted[1] is None and unwanted[2][0, 0] == 0 and unwanted[2][0, 2] == length and not np.any(unwanted[2][:, 0] & navfn.PATH_TRUNCATED)
    for stream in (0, side.cuda_stream):
        assert not _differing(_device(torch, eng, cost, goals, starts, short, want=(True, False, True), stream=stream)[0], unwanted, short)
    got = eng.navfn(cost, goals, starts, short, want=(True, False, True))
    assert got[1] is None and got[0].tobytes() == unwanted[0].tobytes() and got[2].tobytes() == unwanted[2].tobytes()
    exact = dataclasses.replace(P0, max_path=length)
    want = navfn.reference(cost, goals, starts, exact)
    assert want[2][0, 0] == 0
    assert not _differing(_device(torch, eng, cost, goals, starts, exact)[0], want, exact)
    one = eng.navfn(cost[0], goals[0], starts[0], P0)                           # a 2-D grid in, 2-D maps out
    assert one[0].shape == (gh, gw) and one[2].shape == (5,) and np.array_equal(one[2], full[0]) and one[3] >= 1


@pytest.mark.gpu
def test_lethal_cost_and_neutral_move_the_field(eng):
    import torch
    gw, gh = TW + 3, TH + 2
    rng = np.random.default_rng(5)
    cost = rng.integers(0, 256, (2, gh, gw)).astype(np.uint8)
    cost[rng.random((2, gh, gw)) < 0.5] = 0
    cost[:, 0, 0] = 0
    goals, starts = np.array([[0, 0], [0, 0]], np.int32), np.array([[gw - 1, gh - 1], [gw - 1, 0]], np.int32)
    seen = set()
    for kw in (dict(lethal_cost=100), dict(lethal_cost=255), dict(neutral=1), dict(neutral=255, lethal_cost=255, unknown_cost=252, flags=1)):
        p = dataclasses.replace(P0, **kw)
        want = navfn.reference(cost, goals, starts, p)
        assert not _differing(_device(torch, eng, cost, goals, starts, p)[0], want, p), kw
        seen.add(want[0].tobytes())
    assert len(seen) == 4


@pytest.mark.gpu
def test_navfn_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread plans (ctypes drops the GIL): the maps of both equal the serial run's."""
    p, cost, goals, starts, want = _winding()
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=MAX_BATCH) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, done = [], []

        def work():
            try:
                for _ in range(6):
                    got = e.navfn(cost, goals, starts, p)
                    if any(g.tobytes() != w_.tobytes() for g, w_ in zip(got[:3], want)):
                        errors.append("outputs differ")
                    done.append(1)
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
        assert not t.is_alive() and not errors and len(done) == 6, errors


def _scene_params(raw, cam, out_scale=None):
    """obstacle parameters that make something of the engine's own maps, whatever its synthetic weights give: a grid fitted to
    the points under a level mount, and an inflation of 1.2 cells inside 3"""
    kw = {} if out_scale is None else dict(out_scale=out_scale)
    level = obstacles.mount(t=(0.0, 0.0, 0.3))
    xb, yb, zb = obstacles.base_points(raw, cam, ObstacleParams(base_from_cam=level), **kw)
    ok = np.isfinite(xb)
    assert ok.sum() > 500, "the engine's maps hold too few measurements"
    pc = lambda a, v: float(np.float32(np.percentile(a[ok].astype(np.float64), v)))      # noqa: E731
    x0, x1, y0, y1 = pc(xb, 5), pc(xb, 95), pc(yb, 5), pc(yb, 95)
    cell = float(np.float32(max((x1 - x0) / 40, (y1 - y0) / 36, 1e-3)))
    op = ObstacleParams(base_from_cam=level, x_min_m=x0, y_min_m=y0, cell_m=cell, gw=40, gh=36, z_floor_m=-1e3, z_lo_m=pc(zb, 50), z_hi_m=1e3,
                        min_obstacle_hits=1, min_ground_hits=1, beams=0)
    ip = InflateParams(cell_m=cell, inscribed_radius_m=float(np.float32(1.2 * cell)), inflation_radius_m=float(np.float32(3 * cell)),
                       cost_scaling=float(np.float32(0.5 / cell)), lethal_min=100, flags=0)
    return op, ip


@pytest.mark.gpu
def test_end_to_end_on_the_device_from_the_engines_own_map(eng):
    """sn_infer_batch -> sn_obstacles_from_raw -> sn_inflate_grid -> sn_navfn on one stream, fixed rounds: nothing crosses to the
    host in between"""
    import torch
    n = 3
    x = np.stack([synth.model_input_i8(W, H, D, 20 + k) for k in range(n)])
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    raw_host = np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)])
    op, ip = _scene_params(raw_host, cam, eng.out_scale)
    gw, gh = op.gw, op.gh
    p = NavParams(neutral=50, lethal_cost=253, unknown_cost=10, flags=navfn.UNKNOWN_OK, max_rounds=24, max_path=200)
    # the twins first, so that goal and start can be put on cells that are passable
    T = api.inflate_table(ip)
    occ = np.stack([obstacles.reference(raw_host[k], cam, op, out_scale=eng.out_scale)[0] for k in range(n)])
    cost = inflate.reference(occ, ip, T)[0]
    passable = navfn.weights(cost, p) > 0
    goals, starts = [], []
    for k in range(n):      # the scene is in pieces: of a few candidate goals the one that reaches most, and the cell furthest from it
        ys, xs = np.nonzero(passable[k])
        assert ys.size > 50
        fields = [(navfn.reference(cost[k], [(xs[i], ys[i])], None, p)[0][0], i) for i in range(0, ys.size, max(ys.size // 8, 1))]
        field, i = max(fields, key=lambda f: int((f[0] != INF).sum()))
        sy, sx = np.unravel_index(int(np.where(field == INF, 0, field).argmax()), field.shape)
        goals.append((xs[i], ys[i])), starts.append((sx, sy))
    goals, starts = np.array(goals, np.int32), np.array(starts, np.int32)
    want = navfn.reference(cost, goals, starts, p)
    print("end to end stats:", want[2].tolist())
    assert np.any((cost > 0) & (cost < 253)) and np.any(cost >= 253) and np.any(want[2][:, 2] > 5)      # a scene, not an empty map
    d_in = torch.from_numpy(x).cuda()
    d_raw = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    d_occ = torch.full((n * gw * gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_cost = torch.full((n * gw * gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_goals, d_starts = torch.from_numpy(goals).cuda(), torch.from_numpy(starts).cuda()
    outs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, gw, gh, p)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.infer_device(n, d_in.data_ptr(), d_raw.data_ptr(), 0, stream=st.cuda_stream)
    eng.obstacles_device(n, d_raw.data_ptr(), cam, op, occ_ptr=d_occ.data_ptr(), stream=st.cuda_stream)
    eng.inflate_device(n, d_occ.data_ptr(), gw, gh, ip, cost_ptr=d_cost.data_ptr(), stream=st.cuda_stream)
    rounds = eng.navfn_device(n, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), d_starts.data_ptr(), p, *[o.data_ptr() for o in outs],
                              stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert rounds == -1
    assert d_occ.cpu().numpy().view(np.int8).tobytes() == occ.tobytes() and d_cost.cpu().numpy().tobytes() == cost.tobytes()
    assert not _differing([o.cpu().numpy().tobytes() for o in outs], want, p)      # 2 x 2 tiles settle well within 24 rounds


@pytest.mark.gpu
def test_argument_errors_change_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    gw, gh = TW + 9, TH + 5
    cost, goals, starts, _ = _fields(gw, gh, seed=3)
    n = 4
    cost, goals, starts = cost[:n], goals[:n], starts[:n]
    p = dataclasses.replace(P0, max_path=100)
    want = navfn.reference(cost, goals, starts, p)
    c_p = api.nav_params(p)
    sizes = _sizes(MAX_BATCH, gw, gh, p)
    d_cost = torch.from_numpy(cost.copy()).cuda()
    d_goals, d_starts = torch.from_numpy(goals.copy()).cuda(), torch.from_numpy(starts.copy()).cuda()
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [b.data_ptr() + GUARD for b in bufs]
    rounds = C.c_int(-7)
    torch.cuda.synchronize()

    def failed(rc):
        msg = lib.sn_last_error(hnd).decode()
        return rc == ERR_ARG and msg.startswith("sn_navfn: ") and len(msg) > len("sn_navfn: ") and rounds.value == -7

    def call(n=n, c=None, gw=gw, gh=gh, g=None, s=None, prm=c_p, out=None, mem=api.SN_MEM_DEVICE, h=hnd):
        out = ptr if out is None else out
        return lib.sn_navfn(h, n, (d_cost.data_ptr() if c is None else c) or None, gw, gh, (d_goals.data_ptr() if g is None else g) or None,
                            (d_starts.data_ptr() if s is None else s) or None, None if prm is None else C.byref(prm),
                            *[v or None for v in out], C.byref(rounds), mem, None)

    bad_p = {k: api.nav_params(dataclasses.replace(p, **kw)) for k, kw in
             {"neutral 0": dict(neutral=0), "neutral 256": dict(neutral=256), "lethal 0": dict(lethal_cost=0), "lethal 256": dict(lethal_cost=256),
              "unknown 253": dict(unknown_cost=253), "unknown -1": dict(unknown_cost=-1), "flags 2": dict(flags=2), "flags 3": dict(flags=3),
              "rounds -1": dict(max_rounds=-1), "max_path -1": dict(max_path=-1), "path with max_path 0": dict(max_path=0)}.items()}
    bad = {"n = 0": dict(n=0), "n < 0": dict(n=-3), "n > max_batch": dict(n=MAX_BATCH + 1), "null cost": dict(c=0), "null goals": dict(g=0),
           "null params": dict(prm=None), "gw 0": dict(gw=0), "gh 0": dict(gh=0), "gw 4097": dict(gw=4097), "gh < 0": dict(gh=-1),
           "gw * gh > 2^20": dict(n=1, gw=1025, gh=1024), "bad mem": dict(mem=7), "no outputs": dict(out=[0, 0, 0]),
           "path without starts": dict(s=0), "goals misaligned": dict(g=d_goals.data_ptr() + 2), "starts misaligned": dict(s=d_starts.data_ptr() + 1),
           "potential misaligned": dict(out=[ptr[0] + 2, ptr[1], ptr[2]]), "path misaligned": dict(out=[ptr[0], ptr[1] + 1, ptr[2]]),
           "stats misaligned": dict(out=[ptr[0], ptr[1], ptr[2] + 2]),
           "potential is cost": dict(out=[d_cost.data_ptr(), ptr[1], ptr[2]]), "stats overlaps cost": dict(out=[ptr[0], ptr[1], d_cost.data_ptr() + 4]),
           "path overlaps goals": dict(out=[ptr[0], d_goals.data_ptr(), ptr[2]]), "stats overlaps starts": dict(out=[ptr[0], ptr[1], d_starts.data_ptr() + 4]),
           "goals overlap starts": dict(s=d_goals.data_ptr() + 8), "potential overlaps path": dict(out=[ptr[1] + 8, ptr[1], ptr[2]]),
           "potential overlaps stats": dict(out=[ptr[0], ptr[1], ptr[0] + 4 * n * gw * gh - 4]), "path overlaps stats": dict(out=[ptr[0], ptr[1], ptr[1] + 16])}
    bad.update({k: dict(prm=v) for k, v in bad_p.items()})
    for name, kw in bad.items():
        assert failed(call(**kw)), name
    assert call(h=None) == ERR_ARG
    with pytest.raises(api.StereoNetError):
        eng.navfn(cost[0, 0], goals[0], None, p)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5a).all()) for b in bufs), "a refused call wrote something"
    # the bounds themselves are allowed, and the first good call after all that is right
    zero = api.nav_params(dataclasses.replace(p, max_path=0))
    assert call(n=1, gw=gw * gh, gh=1, out=[ptr[0], 0, 0]) == 0 and call(n=1, gw=1, gh=gw * gh, prm=zero, out=[0, 0, ptr[2]]) == 0
    assert call() == 0 and rounds.value >= 1
    torch.cuda.synchronize()
    parts = []
    for b, s in zip(bufs, _sizes(n, gw, gh, p)):
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a)
        parts.append(o[GUARD:GUARD + s].tobytes())
    assert not _differing(parts, want, p)


def _run_harness(tmp_path, tag, model, frames, nframes, goal, env_extra, poses=None):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    args = [os.path.join(COMPAT, "build", "navfn_harness"), model, frames, str(W), str(H), str(nframes), prefix] + \
           (["none", "0"] if goal is None else [repr(float(goal[0])), repr(float(goal[1]))]) + ([poses] if poses else [])
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    kinds = ("grid", "costmap", "inflated", "plan")
    msgs = {kind: [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith(kind + " ")] for kind in kinds}
    order = [l.split()[0] for l in lines if l.split()[0] in kinds]
    return msgs, order, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_plan(weights_blob, tmp_path):
    from hobot_stereonet_amd import build, costmap
    from hobot_stereonet_amd.costmap import CostmapParams
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 3
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(str(tmp_path / "f.bin"))
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0, z_min_m=0.05)
    with api.StereoNetHIP(m) as e:
        raw0 = e.infer_sbs_nv12(sbs)[1].reshape(1, H, W)
        op, ip = _scene_params(raw0, cam)
    op = dataclasses.replace(op, frame="base_footprint")
    cp = CostmapParams(mw=70, mh=33, l_hit=100, l_miss=60, l_min=-150, l_max=250, clear_margin_m=op.cell_m, clear_min_m=0.0, clear_max_m=0.0, frame="map")
    ip = dataclasses.replace(ip, lethal_min=65)
    np_ = NavParams(neutral=20, lethal_cost=255, unknown_cost=40, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=300, goal=(1, 2), start=(3, 4))
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), cp)
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    navfn.save_params(str(tmp_path / "plan.txt"), np_)      # its goal and start lines are the tools': the node reads past them
    T = api.inflate_table(ip)
    cell = float(np.float32(op.cell_m))
    poses = np.array([[(1.5 * k + 0.25) * cell, 0.25 * cell, 0.1 * k] for k in range(nframes)])
    np.savetxt(str(tmp_path / "poses.txt"), poses, fmt="%.17g")
    q = api.costmap_pose_q(cp, op, poses)
    # a goal for the obstacle grid's run: the cell of frame 0's grid that is furthest from the robot's cell by the twin
    occ0 = obstacles.reference(raw0[0], cam, op)[0]
    cost0 = inflate.reference(occ0, ip, T)[0]
    x_min, y_min = float(np.float32(op.x_min_m)), float(np.float32(op.y_min_m))
    cell_of = lambda at, origin, size: int(min(max(np.floor((at - origin) / cell), 0), size - 1))      # noqa: E731
    robot = (cell_of(0.0, x_min, op.gw), cell_of(0.0, y_min, op.gh))
    field = navfn.reference(cost0, [robot], None, np_)[0][0]      # the moves are symmetric in who may pass, so this finds what the robot reaches
    far = np.where(field == INF, 0, field)
    gy, gx = np.unravel_index(int(far.argmax()), far.shape)
    goal_grid = (x_min + (gx + 0.5) * cell, y_min + (gy + 0.5) * cell)
    base = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0", "STEREONET_OBSTACLES": str(tmp_path / "ob.txt"),
            "STEREONET_INFLATE": str(tmp_path / "in.txt")}
    full = dict(base, STEREONET_PLAN=str(tmp_path / "plan.txt"))
    f_bin = str(tmp_path / "f.bin")
    msgs, order, _ = _run_harness(tmp_path, "off", m, f_bin, nframes, goal_grid, base)
    assert not msgs["plan"] and order == ["grid", "inflated"] * nframes          # unset: nothing on the topic
    msgs, order, _ = _run_harness(tmp_path, "nogoal", m, f_bin, nframes, None, full)
    assert not msgs["plan"] and order == ["grid", "inflated"] * nframes          # no goal yet: nothing either
    runs = (("grid", full, goal_grid, "grid", ["grid", "inflated", "plan"], None),
            ("chain", dict(full, STEREONET_COSTMAP=str(tmp_path / "cm.txt")), (1e3, -1e3), "costmap", ["grid", "costmap", "inflated", "plan"],
             str(tmp_path / "poses.txt")))
    for tag, env, goal, suffix, per_frame, poses_file in runs:
        msgs, order, log = _run_harness(tmp_path, tag, m, f_bin, nframes, goal, env, poses_file)
        assert len(msgs["plan"]) == nframes and order == per_frame * nframes and "/stereonet_plan" in log, (tag, order)
        assert log.count("lies outside the grid") == (1 if tag == "chain" else 0)      # clamped per coordinate, logged once
        longest = 0
        for k in range(nframes):
            got, source = msgs["plan"][k], msgs["inflated"][k]
            assert got["frame_id"] == source["frame_id"] and got["stamp"] == source["stamp"] and got["pose_frames_ok"] == "1", (tag, k)
            gw, gh = int(source["width"]), int(source["height"])
            data = np.fromfile(str(tmp_path / f"{tag}.{k}.{suffix}"), np.int8).reshape(1, gh, gw)
            cost = inflate.reference(data, ip, T)[0]
            if tag == "grid":
                ox, oy, at = x_min, y_min, (0.0, 0.0)
            else:
                ox, oy, at = float(q[k, 4]) * cell, float(q[k, 5]) * cell, (poses[k, 0], poses[k, 1])
            g = (cell_of(goal[0], ox, gw), cell_of(goal[1], oy, gh))
            s = (cell_of(at[0], ox, gw), cell_of(at[1], oy, gh))
            assert g == ((gx, gy) if tag == "grid" else (gw - 1, 0))
            _, cells, st = navfn.reference(cost, [g], [s], np_)
            length = min(int(st[0, 2]), np_.max_path)
            xy = np.fromfile(str(tmp_path / f"{tag}.{k}.plan"), np.float64).reshape(-1, 2)
            assert int(got["poses"]) == length == xy.shape[0], (tag, k, st.tolist())
            want_xy = np.stack([ox + (cells[0, :length, 0] + 0.5) * cell, oy + (cells[0, :length, 1] + 0.5) * cell], 1)
            assert xy.tobytes() == want_xy.tobytes(), (tag, k)                     # cell centres in metres, the same doubles
            longest = max(longest, length)
        assert longest > 1, tag      # every cell is passable under these parameters: each run publishes real paths
    # without the inflated grid, or with a file the stage refuses, the node is as it is without the variable
    env = {k: v for k, v in full.items() if k != "STEREONET_INFLATE"}
    msgs, order, log = _run_harness(tmp_path, "alone", m, f_bin, nframes, goal_grid, env)
    assert not msgs["plan"] and order == ["grid"] * nframes and log.count("requires STEREONET_INFLATE") == 1 and log.count("no plan") == 1
    navfn.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(np_, neutral=0))
    msgs, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, goal_grid, dict(base, STEREONET_PLAN=str(tmp_path / "bad.txt")))
    assert not msgs["plan"] and order == ["grid", "inflated"] * nframes and log.count("no plan") == 1
    navfn.save_params(str(tmp_path / "huge.txt"), dataclasses.replace(np_, max_path=(1 << 20) + 1))      # no per-frame allocation of that
    msgs, order, log = _run_harness(tmp_path, "huge", m, f_bin, nframes, goal_grid, dict(base, STEREONET_PLAN=str(tmp_path / "huge.txt")))
    assert not msgs["plan"] and order == ["grid", "inflated"] * nframes and log.count("no plan") == 1


@pytest.mark.gpu
def test_filelist_writes_the_plan(model_factory, tmp_path, capsys):
    from hobot_stereonet_amd import filelist, images
    rng = np.random.default_rng(11)
    n, lists = 2, {}
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
        op, ip = _scene_params(e.infer_sbs_nv12(images.sbs_from_eyes(eyes[0], eyes[1], W, H))[1].reshape(1, H, W), cam)
    plan = NavParams(neutral=20, lethal_cost=255, unknown_cost=40, flags=navfn.UNKNOWN_OK, max_path=300, goal=(op.gw - 2, op.gh - 2), start=(1, 1))
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    navfn.save_params(str(tmp_path / "plan.txt"), plan)
    T = api.inflate_table(ip)
    common = ["--model", model, "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120", "--obstacles", str(tmp_path / "ob.txt")]
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--plan", str(tmp_path / "plan.txt")])      # requires --inflate
    navfn.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(plan, flags=4))
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--inflate", str(tmp_path / "in.txt"), "--plan", str(tmp_path / "bad.txt")])
    capsys.readouterr()
    out = str(tmp_path / "run")
    assert filelist.main(common + ["--out", out, "--inflate", str(tmp_path / "in.txt"), "--plan", str(tmp_path / "plan.txt")]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    reached = 0
    for i in range(n):
        raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)
        occ = obstacles.reference(raw, cam, op)[0]
        cost = inflate.reference(occ, ip, T)[0]
        pot, cells, st = navfn.reference(cost, [plan.goal], [plan.start], plan)
        pgm = open(os.path.join(out, f"{i}.plan.pgm"), "rb").read()
        assert pgm == f"P5\n{op.gw} {op.gh}\n255\n".encode() + navfn.scale_potential(pot[0]).tobytes(), i
        length = min(int(st[0, 2]), plan.max_path)
        text = "".join(f"{x} {y}\n" for x, y in cells[0, :length].tolist())
        assert open(os.path.join(out, f"{i}.path.txt")).read() == text, i
        assert [summary["plan"][k][i] for k in navfn.STATS] == st[0].tolist()
        reached += int(st[0, 1])
    assert reached > 0 and summary["frames"] == n
