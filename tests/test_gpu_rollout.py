"""sn_rollout on the MI355X: samples, best and traj equal the numpy twin's (hobot_stereonet_amd/rollout.py) byte for byte, with 16
guard bytes of 0x5a on either side of every wanted output and cost at an odd address: one sample, one step, no footprint; sample
counts around what a workgroup of k_rollout_eval (GROUP) and a stride of k_rollout_best (BEST_THREADS) cover; (step, point) pairs
one below, at and above a wave; 4096 samples; a 1 x 1 grid and one row; n = 1 and n = max_batch; empty, graded, walled, closed,
unknown and unroutable scenes, poses on a cell edge, at negative coordinates and in all four quadrants, a window of one sample;
every subset of the outputs, host mode and device mode on a caller stream; inflate -> navfn -> rollout on one stream from the
engine's own map; beside inference; argument errors; the node's two topics; the filelist tool.

No tolerance appears: the contract is the same bytes.  The twin is fed the library's tables."""
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

from hobot_stereonet_amd import api, inflate, navfn, obstacles, rollout, synth, weights
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.navfn import NavParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera
from hobot_stereonet_amd.rollout import COLLISION, INF, VALID, RolloutParams

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
MAX_BATCH = 10
GUARD = 16
ERR_ARG = -1      # SN_ERR_ARG (include/stereonet_hip.h)
NAMES = ("samples", "best", "traj")
ALL = (True, True, True)
CELL = 0.05
# 5 x 7 samples, mirrored in w; 7 steps of 11 points: 77 (step, point) pairs, two passes of a wave
P0 = RolloutParams(cell_m=CELL, v_min=0.0, v_max=0.6, nv=5, w_min=-1.5, w_max=1.5, nw=7, sim_time_s=1.0, steps=6, lethal_cost=254,
                   centre_lethal_cost=253, unknown_cost=9, flags=0, w_goal=3, w_occ=2)
FP0 = rollout.rectangle_footprint(0.3, 0.2, 0.1)
NAV = NavParams(neutral=50, lethal_cost=253, unknown_cost=30, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=1)


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


def _sizes(n, p):
    return (8 * n * p.nv * p.nw, 32 * n, 12 * n * (p.steps + 1))


def _expected(want):
    """the twin's outputs as the bytes the call must leave in 0x5a-filled buffers: a map without a valid sample has no traj"""
    samples, best, traj = want
    raw = traj.copy()
    raw[(best[:, 0] & rollout.NO_VALID) != 0] = 0x5a5a5a5a
    return [samples.tobytes(), best.tobytes(), raw.tobytes()]


def _device(torch, eng, cost, pot, q, win, p, fp, want=ALL, stream=0):
    """device mode: cost uploaded to an odd address, every wanted output between GUARD bytes of 0x5a in a buffer of its own ->
    the three outputs as bytes, None where not wanted, after checking the guards"""
    n, gh, gw = cost.shape
    d_cost = torch.zeros(cost.size + 1, dtype=torch.uint8, device="cuda")
    d_cost[1:] = torch.from_numpy(np.array(cost).reshape(-1)).cuda()
    d_pot = torch.from_numpy(np.array(pot).view(np.int32)).cuda()
    d_q = torch.from_numpy(np.array(q, np.int32)).cuda()
    d_win = None if win is None else torch.from_numpy(np.array(win, np.int32)).cuda()
    sizes = _sizes(n, p)
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(sizes, want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + GUARD if b is not None else 0 for b in bufs]
    assert d_cost.data_ptr() % 2 == 0
    eng.rollout_device(n, d_cost.data_ptr() + 1, d_pot.data_ptr(), gw, gh, d_q.data_ptr(), p, fp, 0 if d_win is None else d_win.data_ptr(),
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
    return parts


def _differing(got, want):
    """the names of the outputs whose bytes differ from the twin's"""
    return [name for name, g, w_ in zip(NAMES, got, _expected(want)) if g is not None and g != w_]


def _reasons(samples):
    return samples[..., 1] >> 8 & 0xff


def _steps(samples):
    return samples[..., 1] >> 16


def _field(cost, goal):
    """sn_navfn's potential of (n, gh, gw) grids by its twin, one goal for all"""
    return navfn.reference(cost, [goal] * cost.shape[0], None, NAV)[0]


def _case(cost, pot, poses, p=P0, fp=FP0, win=None):
    """-> what a call takes: the library's tables and quantised poses (origin at the grid's corner) with the arrays"""
    cost = np.ascontiguousarray(cost, np.uint8)
    cost = cost[None] if cost.ndim == 2 else cost
    pot = np.ascontiguousarray(pot, np.uint32).reshape(cost.shape)
    q = api.rollout_pose_q(p.cell_m, 0.0, 0.0, np.asarray(poses, np.float64).reshape(-1, 3))
    centres, offsets = api.rollout_tables(p, fp)
    win = None if win is None else np.asarray(win, np.int32).reshape(-1, 4)
    return dict(cost=cost, pot=pot, q=q, win=win, p=p, fp=np.asarray(fp, np.float32).reshape(-1, 2), tables=(centres, offsets))


def _twin(c):
    return rollout.reference(c["cost"], c["pot"], c["q"], c["win"], c["p"], *c["tables"])


def _run(torch, eng, c, want=ALL, stream=0):
    return _device(torch, eng, c["cost"], c["pot"], c["q"], c["win"], c["p"], c["fp"], want, stream)


GW, GH = 96, 64
MID = (GW * CELL / 2, GH * CELL / 2)


@functools.lru_cache(maxsize=None)
def _scenes():
    """name -> (case, the twin's answer), on 96 x 64 cells of 5 cm; every scene asserts on the twin's own answer that it holds
    what it is meant to exercise.  Shared by the tests and never changed."""
    rng = np.random.default_rng(21)
    out = {}

    def add(name, c, check):
        want = _twin(c)
        assert check(want), (name, want[1].tolist())
        for a in (c["cost"], c["pot"], c["q"]) + want:
            a.setflags(write=False)
        out[name] = (c, want)

    xs = np.arange(GW, dtype=np.uint32)
    # empty and uniform, a potential that depends on x alone, yaw 0: a sample and its mirror in w end on the same column, so every
    # mirrored pair ties and the lower s must win; v = 0 ties across all w as well
    empty = np.zeros((1, GH, GW), np.uint8)
    ramp = np.broadcast_to((GW - 1 - xs) * 250, (1, GH, GW))
    even = dataclasses.replace(P0, nw=6)      # no straight sample: the best one has a mirror image
    c = _case(empty, ramp, [(1.0, MID[1], 0.0)], p=even)

    def ties(want):
        s, b, _ = want
        score = even.w_goal * s[0, :, 0].astype(np.int64) + even.w_occ * (s[0, :, 1] & 0xff)
        same = np.nonzero((_reasons(s[0]) == VALID) & (score == score[b[0, 1]]))[0]
        iv, iw = divmod(int(b[0, 1]), even.nw)
        return b[0, 4] == 30 and same.size >= 2 and same[0] == b[0, 1] and iv * even.nw + (even.nw - 1 - iw) in same and iw < even.nw // 2
    add("empty", c, ties)
    # random graded costs and a random potential, the same map under yaw in all four quadrants
    graded = rng.integers(0, 253, (1, GH, GW)).astype(np.uint8).repeat(4, 0)
    noise = rng.integers(0, 1 << 20, (1, GH, GW)).astype(np.uint32).repeat(4, 0)
    c = _case(graded, noise, [(MID[0], MID[1], a) for a in (0.6, 2.2, -2.5, -0.7)])
    add("graded", c, lambda w_: np.all(w_[1][:, 4] == 35) and len(set(w_[1][:, 1].tolist())) > 1 and np.all((w_[0][..., 1] & 0xff) > 0))
    # a wall ahead with a gap: straight arcs pass, wide ones hit it mid-arc and at the last step; and a potential from a goal behind it
    wall = np.zeros((1, GH, GW), np.uint8)
    wall[0, :, 34] = 254
    wall[0, GH // 2 - 4:GH // 2 + 5, 34] = 0
    c = _case(wall, _field(wall, (GW - 2, GH // 2)), [(1.3, MID[1], 0.0)])

    def walled(want):
        s, b, _ = want
        st = _steps(s[0])[_reasons(s[0]) == COLLISION]
        return b[0, 4] > 0 and b[0, 5] > 0 and np.any(st == P0.steps) and np.any((st > 0) & (st < P0.steps))
    add("wall", c, walled)
    # the robot stands on a lethal cell: everything collides at step 0, no valid sample, traj untouched
    shut = np.zeros((1, GH, GW), np.uint8)
    shut[0, GH // 2 + 2, 23] = 254      # under the front left corner of the footprint
    c = _case(shut, _field(shut, (GW - 2, GH // 2)), [(1.0, MID[1], 0.0)])
    add("closed", c, lambda w_: w_[1][0].tolist() == [1, INF, INF, INF, 0, 35, 0, 0] and np.all(_steps(w_[0]) == 0))
    # unknown cells, under both flag values
    fog = rng.choice(np.array([0, 40, 255], np.uint8), (1, GH, GW), p=(0.9, 0.07, 0.03))
    fog[0, GH // 2 - 4:GH // 2 + 5, 14:27] = 0
    for flags in (0, rollout.UNKNOWN_OK):
        p = dataclasses.replace(P0, flags=flags)
        c = _case(fog, _field(np.where(fog == 255, 0, fog), (GW - 2, GH // 2)), [(1.0, MID[1], 0.3)], p=p)
        if flags:
            add("unknown ok", c, lambda w_: w_[1][0, 4] == 35 and np.any((w_[0][0, :, 1] & 0xff) == 9))
        else:
            add("unknown", c, lambda w_: w_[1][0, 4] > 0 and w_[1][0, 5] > 0)
    # free cells without a route: the potential is infinite right of column 30
    cut = np.array(ramp)
    cut[:, :, 31:] = INF
    add("no route", _case(empty, cut, [(1.0, MID[1], 0.0)]), lambda w_: w_[1][0, 6] > 0 and w_[1][0, 4] > 0 and w_[1][0, 5] == 0)
    # the floor of >> 8: a centre half a cell left of the grid (cell -1, not 0) on a cell edge in y; the grid's corner itself with
    # the footprint half outside; and without a footprint the corner itself
    c = _case(empty.repeat(2, 0), ramp.repeat(2, 0), [(-CELL / 2, 10 * CELL, 0.0), (0.0, 0.0, math.pi / 4)])
    add("outside", c, lambda w_: np.all(w_[1][:, 5] == 35) and np.all(_steps(w_[0]) == 0) and c["q"][:, :2].tolist() == [[-128, 2560], [0, 0]])
    c = _case(empty, ramp, [(0.0, 0.0, 0.0)], fp=())      # along the grid's edge: an arc that turns right leaves at once
    add("corner", c, lambda w_: w_[1][0, 4] > 0 and w_[1][0, 5] > 0 and w_[2][0, 0].tolist() == [0, 0, 0] and w_[2][0, -1, 1] >= 0)
    # a window that leaves one sample
    c = _case(graded[:2], noise[:2], [(MID[0], MID[1], 1.0), (MID[0], MID[1], 4.0)], win=[(2, 2, 3, 3), (4, 4, 0, 0)])
    add("window", c, lambda w_: w_[1][:, 1].tolist() == [2 * 7 + 3, 4 * 7] and np.all(w_[1][:, 7] == 34) and np.all(w_[1][:, 4] == 1))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "graded", "wall", "closed", "unknown", "unknown ok", "no route", "outside", "corner", "window"])
def test_scenes(eng, name):
    import torch
    c, want = _scenes()[name]
    got = _run(torch, eng, c)
    bad = _differing(got, want)
    assert not bad, (name, bad, np.frombuffer(got[1], np.uint32).reshape(-1, 8).tolist(), want[1].tolist())
    assert np.all(want[1][:, 4:].sum(1) == c["p"].nv * c["p"].nw)


def _graded(gw, gh, n, seed):
    rng = np.random.default_rng(seed)
    cost = rng.integers(0, 252, (n, gh, gw)).astype(np.uint8)
    spots = rng.random((n, gh, gw)) < 0.015
    cost[spots] = rng.choice(np.array([252, 253, 254, 255], np.uint8), int(spots.sum()))
    pot = rng.integers(0, 1 << 24, (n, gh, gw)).astype(np.uint32)
    pot[rng.random((n, gh, gw)) < 0.05] = INF
    return cost, pot


# what the kernels' loops and grids turn on: S against a workgroup of k_rollout_eval (GROUP samples of one iw) and a stride of
# k_rollout_best, (T + 1) * (nf + 1) against a wave, the largest S
G, B, LANES = rollout.GROUP, rollout.BEST_THREADS, rollout.WAVE
SHAPES = {"one sample, one step, no footprint": (1, 1, 1, 0),
          "nv one below a workgroup": (G - 1, 3, 2, 3), "nv a workgroup": (G, 1, 2, 3), "nv one above a workgroup": (G + 1, 3, 2, 3),
          "S one below a stride of best": (15, 17, 1, 1), "S a stride of best": (16, 16, 1, 1), "S above a stride of best": (6, 43, 1, 1),
          "pairs one below a wave": (3, 5, 6, 8), "pairs a wave": (3, 5, 7, 7), "pairs one above a wave": (3, 5, 4, 12),
          "the most pairs": (2, 3, rollout.MAX_STEPS, rollout.MAX_POINTS), "4096 samples": (64, 64, 1, 1)}
assert B == 256 and LANES == 64 and [(t + 1) * (f + 1) for _, _, t, f in list(SHAPES.values())[7:10]] == [63, 64, 65]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sample_and_pair_counts(eng, shape):
    import torch
    nv, nw, T, nf = SHAPES[shape]
    gw, gh, n = 37, 29, 3
    p = dataclasses.replace(P0, nv=nv, nw=nw, steps=T, flags=rollout.UNKNOWN_OK, lethal_cost=253, centre_lethal_cost=252)
    ang = np.linspace(0, 2 * math.pi, nf, endpoint=False)
    fp = np.stack([0.12 * np.cos(ang), 0.08 * np.sin(ang)], 1).astype(np.float32)
    cost, pot = _graded(gw, gh, n, seed=nv * 1000 + nw * 10 + T)
    c = _case(cost, pot, [(0.9, 0.7, 0.4), (0.5, 0.9, -1.9), (1.2, 0.3, 2.8)], p=p, fp=fp)
    want = _twin(c)
    assert want[1][:, 4].sum() > 0 and (nv * nw == 1 or want[1][:, 5].sum() > 0), want[1].tolist()
    assert not _differing(_run(torch, eng, c), want), shape


@pytest.mark.gpu
def test_small_grids_and_batches(eng):
    import torch
    # one cell: only the samples that stay inside it survive (v = 0 and nothing else with no footprint)
    p = dataclasses.replace(P0, centre_lethal_cost=255)
    c = _case(np.full((1, 1, 1), 3, np.uint8), np.full((1, 1, 1), 77, np.uint32), [(CELL / 2, CELL / 2, 1.0)], p=p, fp=())
    want = _twin(c)
    assert want[1][0, 4] == P0.nw and want[1][0, 5] == 35 - P0.nw and want[1][0, 1] == 0 and want[1][0, 2] == 3 * 77 + 2 * 3
    assert not _differing(_run(torch, eng, c), want)
    # one row: the robot drives along it, whatever turns leaves it
    row = np.zeros((1, 1, 40), np.uint8)
    row[0, 0, 30:] = 200
    c = _case(row, np.arange(40, dtype=np.uint32)[::-1].reshape(1, 1, 40) * 300, [(0.2, CELL / 2, 0.0)], fp=())
    want = _twin(c)
    assert want[1][0, 4] >= P0.nv and want[1][0, 5] > 0 and want[1][0, 1] == (P0.nv - 1) * P0.nw + P0.nw // 2
    assert not _differing(_run(torch, eng, c), want)
    # n = max_batch: a pose and a window per map; and every map of it alone (n = 1) gives its own rows
    cost, pot = _graded(61, 47, MAX_BATCH, seed=8)
    poses = [(0.6 + 0.15 * k, 1.1 + 0.02 * k, 0.7 * k) for k in range(MAX_BATCH)]
    wins = [(k % 3, 3, 0, 6 - k % 4) for k in range(MAX_BATCH)]
    c = _case(cost, pot, poses, win=wins)
    want = _twin(c)
    assert np.all(want[1][:, 7] > 0) and want[1][:, 4].sum() > 0 and want[1][:, 5].sum() > 0
    assert not _differing(_run(torch, eng, c), want)
    for k in (0, MAX_BATCH - 1):
        one = _case(cost[k], pot[k], [poses[k]], win=[wins[k]])
        alone = _twin(one)
        assert all(a[0].tobytes() == w_[k].tobytes() for a, w_ in zip(alone, want))
        assert not _differing(_run(torch, eng, one), alone)


@pytest.mark.gpu
def test_every_subset_of_the_outputs_in_both_memory_modes(eng):
    import torch
    side = torch.cuda.Stream()
    scenes = _scenes()
    for name in ("wall", "closed", "window"):
        c, want = scenes[name]
        for sub in itertools.product((False, True), repeat=3):
            if not any(sub):
                continue
            for stream in (0, side.cuda_stream):                                # the lane's stream | a caller stream
                assert not _differing(_run(torch, eng, c, want=sub, stream=stream), want), (name, sub, stream)
            got = eng.rollout(c["cost"], c["pot"], c["q"], c["p"], c["fp"], c["win"], want=sub)      # host mode
            assert [g is not None for g in got] == list(sub), sub
            for label, g, w_ in zip(NAMES, got, want):
                assert g is None or (g.dtype == w_.dtype and g.tobytes() == w_.tobytes()), (name, sub, label)
    c, want = scenes["empty"]
    one = eng.rollout(c["cost"][0], c["pot"][0], c["q"][0], c["p"], c["fp"])   # a 2-D grid in, the leading n dropped
    assert one[0].shape == (30, 2) and one[1].shape == (8,) and one[2].shape == (7, 3) and np.array_equal(one[1], want[1][0])
    # the footprint a parameter block carries is the one used when none is given
    carried = dataclasses.replace(c["p"], footprint=tuple(map(tuple, c["fp"].tolist())))
    assert eng.rollout(c["cost"], c["pot"], c["q"], carried)[0].tobytes() == want[0].tobytes()


@pytest.mark.gpu
def test_another_parameter_block_replaces_the_tables(eng):
    """the lane keeps the tables of the last (parameters, footprint) pair: alternating pairs, each must get its own"""
    import torch
    c, want = _scenes()["wall"]
    wide = rollout.rectangle_footprint(0.5, 0.4, 0.1)
    slow = dataclasses.replace(c["p"], v_max=0.3)
    cases = [(c, want)]
    for p, fp in ((c["p"], wide), (slow, c["fp"])):
        other = dict(c, p=p, fp=np.asarray(fp, np.float32), tables=api.rollout_tables(p, fp))
        cases.append((other, _twin(other)))
    assert len({w_[0].tobytes() for _, w_ in cases}) == 3
    for case, w_ in cases + cases[::-1]:
        assert not _differing(_run(torch, eng, case), w_)


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
    """sn_infer_batch -> sn_obstacles_from_raw -> sn_inflate_grid -> sn_navfn (fixed rounds) -> sn_rollout on one stream: nothing
    crosses to the host in between, and the outputs equal the host-mode chain's and the twin's"""
    import torch
    n = 3
    x = np.stack([synth.model_input_i8(W, H, D, 20 + k) for k in range(n)])
    cam = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
    raw_host = np.stack([eng.infer(x[k])[1].reshape(H, W) for k in range(n)])
    op, ip = _scene_params(raw_host, cam, eng.out_scale)
    gw, gh, cell = op.gw, op.gh, op.cell_m
    nav = NavParams(neutral=50, lethal_cost=253, unknown_cost=10, flags=navfn.UNKNOWN_OK, max_rounds=24, max_path=1)
    # the host-mode chain first, so that goal and pose can be put on cells that are passable
    occ = eng.obstacles(raw_host, cam, op)[0].reshape(n, gh, gw)
    cost = eng.inflate(occ, ip)[0]
    passable = navfn.weights(cost, nav) > 0
    goals, poses = [], []
    for k in range(n):
        ys, xs = np.nonzero(passable[k])
        assert ys.size > 50
        goals.append((xs[-1], ys[-1]))
        i = ys.size // 3
        poses.append(((xs[i] + 0.5) * cell, (ys[i] + 0.5) * cell, 0.8 * k))
    goals = np.array(goals, np.int32)
    pot = eng.navfn(cost, goals, None, nav, want=(True, False, False))[0]
    p = dataclasses.replace(P0, cell_m=cell, v_max=float(np.float32(6 * cell)), flags=rollout.UNKNOWN_OK, unknown_cost=10)
    fp = rollout.rectangle_footprint(1.5 * cell, 1.0 * cell, 0.5 * cell)
    q = api.rollout_pose_q(cell, 0.0, 0.0, poses)
    host = eng.rollout(cost, pot, q, p, fp)
    want = rollout.reference(cost, pot, q, None, p, *api.rollout_tables(p, fp))
    print("end to end best:", want[1].tolist())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, want))
    assert want[1][:, 4].sum() > 0 and want[1][:, 4].sum() + want[1][:, 5].sum() + want[1][:, 6].sum() == n * 35
    d_in = torch.from_numpy(x).cuda()
    d_raw = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    d_occ = torch.full((n * gw * gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_cost = torch.full((n * gw * gh,), 0x5a, dtype=torch.uint8, device="cuda")
    d_pot = torch.full((n * gw * gh,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_goals, d_q = torch.from_numpy(goals).cuda(), torch.from_numpy(q).cuda()
    outs = [torch.full((s,), 0x5a, dtype=torch.uint8, device="cuda") for s in _sizes(n, p)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.infer_device(n, d_in.data_ptr(), d_raw.data_ptr(), 0, stream=st.cuda_stream)
    eng.obstacles_device(n, d_raw.data_ptr(), cam, op, occ_ptr=d_occ.data_ptr(), stream=st.cuda_stream)
    eng.inflate_device(n, d_occ.data_ptr(), gw, gh, ip, cost_ptr=d_cost.data_ptr(), stream=st.cuda_stream)
    assert eng.navfn_device(n, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), 0, nav, potential_ptr=d_pot.data_ptr(), stream=st.cuda_stream) == -1
    eng.rollout_device(n, d_cost.data_ptr(), d_pot.data_ptr(), gw, gh, d_q.data_ptr(), p, fp, 0, *[o.data_ptr() for o in outs], stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert d_cost.cpu().numpy().tobytes() == cost.tobytes() and d_pot.cpu().numpy().view(np.uint32).tobytes() == pot.tobytes()
    assert not _differing([o.cpu().numpy().tobytes() for o in outs], want)


@pytest.mark.gpu
def test_rollout_beside_submit_and_wait(model_factory):
    """sn_submit tickets in flight while another thread rolls out (ctypes drops the GIL): the outputs of both equal the serial run's."""
    c, want = _scenes()["wall"]
    xs = [synth.model_input_i8(W, H, D, s) for s in range(4)]
    with api.StereoNetHIP(model_factory(W, H, D), task_num=4, max_batch=MAX_BATCH) as e:
        serial = [e.infer(x)[1] for x in xs]
        errors, done = [], []

        def work():
            try:
                for _ in range(6):
                    got = e.rollout(c["cost"], c["pot"], c["q"], c["p"], c["fp"])
                    if any(g.tobytes() != w_.tobytes() for g, w_ in zip(got, want)):
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


@pytest.mark.gpu
def test_argument_errors_change_nothing(eng):
    import torch
    lib, hnd = eng._lib, eng._h
    cost, pot = _graded(41, 37, 4, seed=3)
    n, gh, gw = cost.shape
    case = _case(cost, pot, [(1.0, 0.9, 0.5 * k) for k in range(n)], win=[(0, 4, 0, 6)] * n)
    want = _twin(case)
    p, fp = case["p"], case["fp"]
    c_p = api.rollout_params(p)
    sizes = _sizes(MAX_BATCH, p)
    d_cost, d_pot = torch.from_numpy(cost.copy()).cuda(), torch.from_numpy(pot.view(np.int32).copy()).cuda()
    d_q, d_win = torch.from_numpy(case["q"].copy()).cuda(), torch.from_numpy(case["win"].copy()).cuda()
    bufs = [torch.full((s + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [b.data_ptr() + GUARD for b in bufs]
    nan_fp = fp.copy()
    nan_fp[3, 1] = np.nan
    far_fp = fp.copy()
    far_fp[0] = (500.0, 0.0)      # 10 000 cells: beyond 2^21 / 256
    torch.cuda.synchronize()

    def failed(rc):
        msg = lib.sn_last_error(hnd).decode()
        return rc == ERR_ARG and msg.startswith("sn_rollout: ") and len(msg) > len("sn_rollout: ")

    def call(n=n, c=None, pt=None, gw=gw, gh=gh, q=None, win=None, prm=c_p, f=fp, nf=None, out=None, mem=api.SN_MEM_DEVICE, h=hnd):
        out = ptr if out is None else out
        pick = lambda given, dflt: (dflt if given is None else given) or None      # noqa: E731
        return lib.sn_rollout(h, n, pick(c, d_cost.data_ptr()), pick(pt, d_pot.data_ptr()), gw, gh, pick(q, d_q.data_ptr()),
                              pick(win, d_win.data_ptr()), None if prm is None else C.byref(prm), None if f is None else f.ctypes.data,
                              fp.shape[0] if nf is None else nf, *[v or None for v in out], mem, None)

    mods = {"cell 0": dict(cell_m=0.0), "cell nan": dict(cell_m=float("nan")), "cell inf": dict(cell_m=float("inf")), "v inf": dict(v_max=float("inf")),
            "v_max < v_min": dict(v_max=-0.1), "w nan": dict(w_min=float("nan")), "w_max < w_min": dict(w_max=-2.0), "nv 0": dict(nv=0),
            "nv 65": dict(nv=65), "nw 0": dict(nw=0), "nw 65": dict(nw=65), "sim 0": dict(sim_time_s=0.0), "sim < 0": dict(sim_time_s=-1.0),
            "steps 0": dict(steps=0), "steps 65": dict(steps=65), "lethal 0": dict(lethal_cost=0), "lethal 256": dict(lethal_cost=256),
            "centre 0": dict(centre_lethal_cost=0), "centre 256": dict(centre_lethal_cost=256), "unknown -1": dict(unknown_cost=-1),
            "unknown 253": dict(unknown_cost=253), "flags 2": dict(flags=2), "w_goal -1": dict(w_goal=-1), "w_goal 32768": dict(w_goal=32768),
            "w_occ 32768": dict(w_occ=32768), "both weights 0": dict(w_goal=0, w_occ=0), "an arc too long": dict(v_max=500.0, sim_time_s=30.0),
            "too many turns": dict(w_max=3.0e6, sim_time_s=10.0)}
    bad = {"n = 0": dict(n=0), "n < 0": dict(n=-3), "n > max_batch": dict(n=MAX_BATCH + 1), "null cost": dict(c=0), "null potential": dict(pt=0),
           "null poses": dict(q=0), "null params": dict(prm=None), "null footprint": dict(f=None), "nf -1": dict(nf=-1), "nf 65": dict(nf=65),
           "footprint nan": dict(f=nan_fp), "footprint too far": dict(f=far_fp), "gw 0": dict(gw=0), "gh 0": dict(gh=0), "gw 4097": dict(gw=4097),
           "gh < 0": dict(gh=-1), "gw * gh > 2^20": dict(n=1, gw=1025, gh=1024), "bad mem": dict(mem=7), "no outputs": dict(out=[0, 0, 0]),
           "potential misaligned": dict(pt=d_pot.data_ptr() + 2), "poses misaligned": dict(q=d_q.data_ptr() + 1), "window misaligned": dict(win=d_win.data_ptr() + 2),
           "samples misaligned": dict(out=[ptr[0] + 2, ptr[1], ptr[2]]), "best misaligned": dict(out=[ptr[0], ptr[1] + 1, ptr[2]]),
           "traj misaligned": dict(out=[ptr[0], ptr[1], ptr[2] + 2]), "samples is potential": dict(out=[d_pot.data_ptr(), ptr[1], ptr[2]]),
           "best overlaps cost": dict(out=[ptr[0], d_cost.data_ptr() + 4, ptr[2]]), "traj overlaps poses": dict(out=[ptr[0], ptr[1], d_q.data_ptr()]),
           "best overlaps window": dict(out=[ptr[0], d_win.data_ptr() + 4, ptr[2]]), "window overlaps poses": dict(win=d_q.data_ptr() + 8),
           "cost overlaps potential": dict(c=d_pot.data_ptr() + 1), "samples overlap best": dict(out=[ptr[1] + 8, ptr[1], ptr[2]]),
           "best overlaps traj": dict(out=[ptr[0], ptr[2] + 16, ptr[2]])}
    bad.update({k: dict(prm=api.rollout_params(dataclasses.replace(p, **kw))) for k, kw in mods.items()})
    for name, kw in bad.items():
        assert failed(call(**kw)), name
    assert call(h=None) == ERR_ARG
    with pytest.raises(api.StereoNetError):
        eng.rollout(cost[0, 0], pot[0, 0], case["q"][0], p, fp)
    with pytest.raises(api.StereoNetError):
        eng.rollout(cost, pot[:, :-1], case["q"], p, fp)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5a).all()) for b in bufs), "a refused call wrote something"
    # the bounds themselves are allowed, and the first good call after all that is right
    assert call(n=1, gw=gw * gh, gh=1, out=[ptr[0], 0, 0]) == 0 and call(n=1, gw=1, gh=gw * gh, win=0, out=[0, ptr[1], 0]) == 0
    for b in bufs:
        b.fill_(0x5a)
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    parts = []
    for b, s in zip(bufs, _sizes(n, p)):
        o = b.cpu().numpy()
        assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + s:] == 0x5a)
        parts.append(o[GUARD:GUARD + s].tobytes())
    assert not _differing(parts, want)


@pytest.mark.gpu
def test_filelist_writes_the_rollout(model_factory, tmp_path, capsys):
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
    cell = op.cell_m
    plan = NavParams(neutral=20, lethal_cost=255, unknown_cost=40, flags=navfn.UNKNOWN_OK, max_path=300, goal=(op.gw - 2, op.gh - 2), start=(5, 6))
    fp = rollout.rectangle_footprint(1.5 * cell, 1.0 * cell, 0.5 * cell)
    roll = dataclasses.replace(P0, cell_m=cell, v_max=float(np.float32(6 * cell)), lethal_cost=255, centre_lethal_cost=255, flags=rollout.UNKNOWN_OK,
                               unknown_cost=40, footprint=tuple(map(tuple, fp.astype(np.float64).tolist())))
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    navfn.save_params(str(tmp_path / "plan.txt"), plan)
    rollout.save_params(str(tmp_path / "roll.txt"), roll)
    T = api.inflate_table(ip)
    common = ["--model", model, "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120", "--obstacles", str(tmp_path / "ob.txt"),
              "--inflate", str(tmp_path / "in.txt")]
    with pytest.raises(SystemExit):
        filelist.main(common + ["--out", str(tmp_path / "x"), "--rollout", str(tmp_path / "roll.txt")])      # requires --plan
    rollout.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(roll, nv=0))
    rollout.save_params(str(tmp_path / "cell.txt"), dataclasses.replace(roll, cell_m=2 * cell))
    for bad in ("bad.txt", "cell.txt"):
        with pytest.raises(SystemExit):
            filelist.main(common + ["--out", str(tmp_path / "x"), "--plan", str(tmp_path / "plan.txt"), "--rollout", str(tmp_path / bad)])
    capsys.readouterr()
    tables = api.rollout_tables(roll)
    for tag, params, pose in (("start", roll, ((5 + 0.5) * float(np.float32(cell)), (6 + 0.5) * float(np.float32(cell)), 0.0)),
                              ("posed", dataclasses.replace(roll, pose=(7.25 * cell, 9.5 * cell, 0.9)), None)):
        rollout.save_params(str(tmp_path / f"{tag}.txt"), params)
        pose = params.pose if pose is None else pose
        out = str(tmp_path / tag)
        assert filelist.main(common + ["--out", out, "--plan", str(tmp_path / "plan.txt"), "--rollout", str(tmp_path / f"{tag}.txt")]) == 0
        summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        valid = 0
        for i in range(n):
            raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(H, W)
            cost = inflate.reference(obstacles.reference(raw, cam, op)[0], ip, T)[0]
            pot = navfn.reference(cost, [plan.goal], [plan.start], plan)[0]
            q = api.rollout_pose_q(cell, 0.0, 0.0, [pose])
            _, best, traj = rollout.reference(cost, pot, q, None, roll, *tables)
            found = not best[0, 0] & rollout.NO_VALID
            v, w_ = api.rollout_velocity(roll, int(best[0, 1])) if found else (0.0, 0.0)
            text = f"cmd {v!r} {w_!r}\nbest " + " ".join(str(int(x)) for x in best[0]) + "\n"
            text += "".join(f"{x} {y} {a}\n" for x, y, a in traj[0].tolist()) if found else ""
            assert open(os.path.join(out, f"{i}.rollout.txt")).read() == text, (tag, i)
            got = {k: summary["rollout"][k][i] for k in ("v", "w", "score", "valid", "collided", "no_route", "out_of_window")}
            score = int(best[0, 2]) | int(best[0, 3]) << 32
            assert got == dict(v=v, w=w_, score=score if found else None, valid=int(best[0, 4]), collided=int(best[0, 5]), no_route=int(best[0, 6]),
                               out_of_window=0), (tag, i)
            valid += int(best[0, 4])
        assert valid > 0 and summary["frames"] == n, tag


def _run_harness(tmp_path, tag, model, frames, nframes, goal, env_extra, poses=None, velocity=None):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    args = [os.path.join(COMPAT, "build", "rollout_harness"), model, frames, str(W), str(H), str(nframes), str(tmp_path / tag)] + \
           (["none", "0"] if goal is None else [repr(float(goal[0])), repr(float(goal[1]))]) + [poses or "none"] + \
           ([] if velocity is None else [repr(float(velocity[0])), repr(float(velocity[1]))])
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    kinds = ("grid", "costmap", "inflated", "plan", "cmd", "local_plan")
    msgs = {kind: [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith(kind + " ")] for kind in kinds}
    order = [l.split()[0] for l in lines if l.split()[0] in kinds]
    return msgs, order, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_command_and_the_local_plan(weights_blob, tmp_path):
    """STEREONET_ROLLOUT: geometry_msgs/Twist on /stereonet_cmd_vel and nav_msgs/Path on /stereonet_local_plan after /stereonet_plan,
    equal to what the twin makes of the grid the node published, with the window of SetVelocity and a zero Twist without a valid sample"""
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
        op, ip = _scene_params(e.infer_sbs_nv12(sbs)[1].reshape(1, H, W), cam)
    op = dataclasses.replace(op, frame="base_footprint")
    cp = CostmapParams(mw=70, mh=33, l_hit=100, l_miss=60, l_min=-150, l_max=250, clear_margin_m=op.cell_m, clear_min_m=0.0, clear_max_m=0.0, frame="map")
    ip = dataclasses.replace(ip, lethal_min=65)
    plan = NavParams(neutral=20, lethal_cost=255, unknown_cost=40, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=300)
    cell = float(np.float32(op.cell_m))
    fp = rollout.rectangle_footprint(1.5 * cell, 1.0 * cell, 0.5 * cell)
    roll = dataclasses.replace(P0, cell_m=2 * cell, v_max=float(np.float32(6 * cell)), lethal_cost=255, centre_lethal_cost=255, flags=rollout.UNKNOWN_OK,
                               unknown_cost=40, footprint=tuple(map(tuple, fp.astype(np.float64).tolist())), acc=(2 * cell, 1.0, 0.5),
                               pose=(1.0, 2.0, 3.0))      # cell_m and pose are not the node's: it takes the grid's cell and its own pose
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    costmap.save_params(str(tmp_path / "cm.txt"), cp)
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    navfn.save_params(str(tmp_path / "plan.txt"), plan)
    rollout.save_params(str(tmp_path / "roll.txt"), roll)
    far = dataclasses.replace(roll, footprint=roll.footprint + ((200 * cell, 0.0),))      # a point that is never on the grid: no sample is valid
    rollout.save_params(str(tmp_path / "far.txt"), far)
    T = api.inflate_table(ip)
    poses = np.array([[(1.5 * k + 0.25) * cell, 0.25 * cell, 0.1 * k] for k in range(nframes)])
    np.savetxt(str(tmp_path / "poses.txt"), poses, fmt="%.17g")
    x_min, y_min = float(np.float32(op.x_min_m)), float(np.float32(op.y_min_m))
    goal_grid = (x_min + 30.5 * cell, y_min + 20.5 * cell)
    base = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0", "STEREONET_OBSTACLES": str(tmp_path / "ob.txt"),
            "STEREONET_INFLATE": str(tmp_path / "in.txt"), "STEREONET_PLAN": str(tmp_path / "plan.txt")}
    full = dict(base, STEREONET_ROLLOUT=str(tmp_path / "roll.txt"))
    f_bin = str(tmp_path / "f.bin")
    msgs, order, _ = _run_harness(tmp_path, "off", m, f_bin, nframes, goal_grid, base)
    assert not msgs["cmd"] and not msgs["local_plan"] and order == ["grid", "inflated", "plan"] * nframes      # unset: nothing on the topics
    msgs, order, _ = _run_harness(tmp_path, "nogoal", m, f_bin, nframes, None, full)
    assert not msgs["cmd"] and not msgs["local_plan"] and order == ["grid", "inflated"] * nframes             # no goal yet: nothing either
    cell_of = lambda at, origin, size: int(min(max(np.floor((at - origin) / cell), 0), size - 1))      # noqa: E731
    moving = (3 * cell, 0.4)
    # the obstacle grid alone (the robot at the base frame's origin, which need not lie on the grid: the twin says what comes of it);
    # the costmap's window around the robot, with a velocity: every frame has a command, from inside the window; a footprint that
    # never fits: every frame stops
    runs = (("grid", full, goal_grid, "grid", ["grid", "inflated", "plan", "cmd", "local_plan"], None, None, roll),
            ("chain", dict(full, STEREONET_COSTMAP=str(tmp_path / "cm.txt")), (1e3, -1e3), "costmap",
             ["grid", "costmap", "inflated", "plan", "cmd", "local_plan"], str(tmp_path / "poses.txt"), moving, roll),
            ("far", dict(full, STEREONET_ROLLOUT=str(tmp_path / "far.txt")), goal_grid, "grid", ["grid", "inflated", "plan", "cmd", "local_plan"], None,
             None, far))
    for tag, env, goal, suffix, per_frame, poses_file, velocity, params in runs:
        msgs, order, log = _run_harness(tmp_path, tag, m, f_bin, nframes, goal, env, poses_file, velocity)
        assert len(msgs["cmd"]) == len(msgs["local_plan"]) == nframes and order == per_frame * nframes, (tag, order)
        assert "/stereonet_cmd_vel" in log and "/stereonet_local_plan" in log
        moved = 0
        for k in range(nframes):
            got, arc, source = msgs["cmd"][k], msgs["local_plan"][k], msgs["inflated"][k]
            assert arc["frame_id"] == source["frame_id"] and arc["stamp"] == source["stamp"] and arc["pose_frames_ok"] == "1", (tag, k)
            gw, gh, res = int(source["width"]), int(source["height"]), float(np.float32(float(source["resolution"])))
            assert res == cell
            ox, oy = (float(v) for v in source["origin"].split(","))
            data = np.fromfile(str(tmp_path / f"{tag}.{k}.{suffix}"), np.int8).reshape(1, gh, gw)
            cost = inflate.reference(data, ip, T)[0]
            pose = (0.0, 0.0, 0.0) if poses_file is None else tuple(poses[k])
            g = (cell_of(goal[0], ox, gw), cell_of(goal[1], oy, gh))
            s = (cell_of(pose[0], ox, gw), cell_of(pose[1], oy, gh))
            pot = navfn.reference(cost, [g], [s], plan)[0]
            p = dataclasses.replace(params, cell_m=res)
            win = None if velocity is None else rollout.window_from_velocity(p, velocity[0], velocity[1], *p.acc)
            _, best, traj = rollout.reference(cost, pot, api.rollout_pose_q(res, ox, oy, [pose]), win, p, *api.rollout_tables(p))
            xyzw = np.fromfile(str(tmp_path / f"{tag}.{k}.local_plan"), np.float64).reshape(-1, 4)
            assert float(got["rest"]) == 0.0
            if best[0, 0] & rollout.NO_VALID:
                assert float(got["v"]) == 0.0 and float(got["w"]) == 0.0 and arc["poses"] == "0" and xyzw.size == 0, (tag, k)
                continue
            assert (float(got["v"]), float(got["w"])) == api.rollout_velocity(p, int(best[0, 1])), (tag, k, best[0].tolist())
            half = [float(a) / 65536.0 * 3.141592653589793 for a in traj[0, :, 2]]
            want = np.stack([ox + traj[0, :, 0] / 256.0 * res, oy + traj[0, :, 1] / 256.0 * res, [math.sin(a) for a in half],
                             [math.cos(a) for a in half]], 1)
            assert int(arc["poses"]) == p.steps + 1 and xyzw.tobytes() == want.tobytes(), (tag, k)
            assert velocity is None or (best[0, 7] > 0 and win[0] <= best[0, 1] // p.nw <= win[1] and win[2] <= best[0, 1] % p.nw <= win[3])
            moved += 1
        print("node run", tag, "frames with a command:", moved)
        assert tag == "grid" or moved == (0 if tag == "far" else nframes), (tag, moved)
    # without the plan, or with a file the stage refuses, the node is as it is without the variable
    env = {k: v for k, v in full.items() if k != "STEREONET_PLAN"}
    msgs, order, log = _run_harness(tmp_path, "alone", m, f_bin, nframes, goal_grid, env)
    assert not msgs["cmd"] and order == ["grid", "inflated"] * nframes and log.count("requires STEREONET_PLAN") == 1 and log.count("no velocity command") == 1
    for bad in (dataclasses.replace(roll, nv=0), dataclasses.replace(roll, acc=(-1.0, 1.0, 1.0)), dataclasses.replace(roll, footprint=roll.footprint * 7)):
        rollout.save_params(str(tmp_path / "bad.txt"), bad)
        msgs, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, goal_grid, dict(full, STEREONET_ROLLOUT=str(tmp_path / "bad.txt")))
        assert not msgs["cmd"] and not msgs["local_plan"] and order == ["grid", "inflated", "plan"] * nframes and log.count("no velocity command") == 1
