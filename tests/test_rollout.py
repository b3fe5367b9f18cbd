"""The trajectory rollout without a GPU: the vectorised twin (hobot_stereonet_amd/rollout.py) equals a plain loop over Python
integers written from the header, byte for byte; the library's host tables and pose quantisation agree with the Python
restatement within one per entry (two libms), and exactly where no rounding is in play; every refusal, on both sides; the window
helper's edge cases; the footprint helper; the header's constants equal rollout.py's; the parameter file round-trips."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, rollout
from hobot_stereonet_amd.rollout import COLLISION, INF, NO_ROUTE, OUT_OF_WINDOW, VALID, RolloutParams

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
P0 = RolloutParams(cell_m=0.05, v_min=-0.1, v_max=0.5, nv=5, w_min=-1.2, w_max=1.2, nw=7, sim_time_s=1.5, steps=6, lethal_cost=254,
                   centre_lethal_cost=253, unknown_cost=7, flags=0, w_goal=3, w_occ=2)
FP0 = rollout.rectangle_footprint(0.3, 0.2, 0.1)


def _maps(rng, n, gh, gw, dense):
    cost = rng.integers(0, 252, (n, gh, gw)).astype(np.uint8)
    spots = rng.random((n, gh, gw)) < dense
    cost[spots] = rng.choice(np.array([252, 253, 254, 255], np.uint8), int(spots.sum()))
    pot = rng.integers(0, 1 << 30, (n, gh, gw)).astype(np.uint32)
    pot[rng.random((n, gh, gw)) < 0.3] = INF
    return cost, pot


@pytest.mark.parametrize("flags", [0, rollout.UNKNOWN_OK])
def test_twin_equals_the_plain_integer_loop(flags):
    rng = np.random.default_rng(5 + flags)
    seen = np.zeros(4, np.int64)
    steps_seen = set()
    for (gw, gh), nf_fp, lethal in (((40, 30), FP0, 254), ((23, 31), FP0[:3], 200), ((1, 1), FP0[:0], 255), ((50, 1), FP0[:0], 254)):
        p = dataclasses.replace(P0, flags=flags, lethal_cost=lethal, centre_lethal_cost=min(lethal, 253))
        centres, offsets = api.rollout_tables(p, nf_fp)
        cost, pot = _maps(rng, 4, gh, gw, 0.006)
        poses = np.stack([rng.uniform(0.3, 0.7, 4) * gw * 0.05, rng.uniform(0.3, 0.7, 4) * gh * 0.05, rng.uniform(-7, 7, 4)], 1)
        poses[3, :2] = rng.uniform(-0.1, 0.2, 2)                  # near the grid's corner, perhaps outside it
        poses[0] = (gw * 0.025, gh * 0.025, 0.0)
        q = api.rollout_pose_q(p.cell_m, 0.0, 0.0, poses)
        for win in (None, np.array([[1, 3, 2, 5], [0, 4, 0, 6], [2, 2, 6, 6], [3, 1, 0, 6]])):      # the last one is empty
            samples, best, traj = rollout.reference(cost, pot, q, win, p, centres, offsets)
            assert samples.dtype == np.uint32 and best.dtype == np.uint32 and traj.dtype == np.int32
            for k in range(4):
                ls, lb, lt = rollout.loop_reference(cost[k], pot[k], q[k], None if win is None else win[k].tolist(), p, centres, offsets)
                assert samples[k].tolist() == ls and best[k].tolist() == lb, (gw, gh, k)
                assert (lt is None and not traj[k].any() and lb[0] == rollout.NO_VALID) or traj[k].tolist() == lt
                assert sum(lb[4:]) == p.nv * p.nw
            r = samples[..., 1] >> 8 & 0xff
            seen += np.bincount(r.ravel(), minlength=4)
            steps_seen |= set((samples[..., 1] >> 16)[r == COLLISION].tolist())
            assert np.all(samples[..., 0][r != VALID] == INF) and np.all((samples[..., 1] & 0xff)[r != VALID] == 0)
    assert np.all(seen > 20), seen.tolist()                      # every reason class is well populated
    assert {0, P0.steps} <= steps_seen and len(steps_seen) > 3   # collisions at the first, the last and steps in between


def test_library_tables_agree_with_the_restatement():
    for p, fp in ((P0, FP0), (dataclasses.replace(P0, nv=1, nw=1, steps=1), FP0[:0]), (dataclasses.replace(P0, nv=64, nw=64, steps=2), FP0[:2]),
                  (dataclasses.replace(P0, w_min=0.0, w_max=0.0, nw=3, steps=64), rollout.rectangle_footprint(0.6, 0.4, 0.05 * 0.7))):
        centres, offsets = api.rollout_tables(p, fp)
        c2, o2 = rollout.tables(p, fp)
        assert centres.shape == c2.shape == (p.nv * p.nw, p.steps + 1, 3) and offsets.shape == o2.shape == (p.nw, p.steps + 1, len(fp), 2)
        assert centres.dtype == np.int32 and offsets.dtype == np.int32
        assert np.abs(centres[..., :2].astype(np.int64) - c2[..., :2]).max() <= 1
        dbam = (centres[..., 2].astype(np.int64) - c2[..., 2]) & 0xFFFF
        assert np.all((dbam <= 1) | (dbam == 0xFFFF))
        assert offsets.size == 0 or np.abs(offsets.astype(np.int64) - o2).max() <= 1
        # step 0 is the robot where it stands, whatever the sample; a straight sample stays on the axis
        assert not centres[:, 0].any() and np.array_equal(offsets[:, 0], np.broadcast_to(offsets[0, 0], offsets[:, 0].shape))
    centres, _ = api.rollout_tables(P0, FP0)
    straight = centres.reshape(P0.nv, P0.nw, P0.steps + 1, 3)[:, P0.nw // 2]
    assert not straight[..., 1:].any()
    k256 = 256.0 / float(np.float32(P0.cell_m))
    assert straight[-1, -1, 0] == round(float(np.float32(0.5)) * float(np.float32(1.5)) * k256)
    # either output may be left out
    prm, lib = api.rollout_params(P0), api.load_library()
    only = np.empty_like(centres)
    assert lib.sn_rollout_tables(C.byref(prm), FP0.ctypes.data, len(FP0), only.ctypes.data, None) == 0 and np.array_equal(only, centres)
    # the velocities of the lattice
    for s in (0, 9, P0.nv * P0.nw - 1):
        assert api.rollout_velocity(P0, s) == rollout.velocity(P0, s)
    assert api.rollout_velocity(P0, 0) == (float(np.float32(-0.1)), float(np.float32(-1.2)))
    assert rollout.velocity(dataclasses.replace(P0, nv=1, nw=1), 0) == (float(np.float32(-0.1)), float(np.float32(-1.2)))


def test_pose_q_agrees_with_the_restatement():
    rng = np.random.default_rng(2)
    poses = np.stack([rng.uniform(-50, 50, 40), rng.uniform(-50, 50, 40), rng.uniform(-10, 10, 40)], 1)
    got = api.rollout_pose_q(0.05, -3.0, 2.5, poses)
    want = np.stack([rollout.pose_q(0.05, -3.0, 2.5, ps) for ps in poses])
    assert got.dtype == np.int32 and got.shape == (40, 5)
    assert np.abs(got[:, :4].astype(np.int64) - want[:, :4]).max() <= 1
    dbam = (got[:, 4].astype(np.int64) - want[:, 4]) & 0xFFFF
    assert np.all((dbam <= 1) | (dbam == 0xFFFF))
    # exact at yaw 0 and at integer cell coordinates: cell 0.25 m is a power of two, so nothing rounds
    q = api.rollout_pose_q(0.25, -1.0, 0.5, [(0.75, -2.0, 0.0)])
    assert q.tolist() == [[7 * 256, -10 * 256, 1 << 30, 0, 0]] and rollout.pose_q(0.25, -1.0, 0.5, (0.75, -2.0, 0.0)).tolist() == q[0].tolist()
    assert api.rollout_pose_q(0.25, 0.0, 0.0, (0.0, 0.0, math.pi / 2))[2:].tolist() == [0, 1 << 30, 16384]
    assert api.rollout_pose_q(0.25, 0.0, 0.0, (0.0, 0.0, -math.pi / 2))[4] == 49152
    assert api.rollout_pose_q(0.25, 0.0, 0.0, (-0.125, 0.0, 0.0))[0] == -128      # half a cell left of the origin


BAD_PARAMS = {"cell 0": dict(cell_m=0.0), "cell nan": dict(cell_m=float("nan")), "cell inf": dict(cell_m=float("inf")), "v inf": dict(v_max=float("inf")),
              "v_max < v_min": dict(v_max=-0.2), "w nan": dict(w_min=float("nan")), "w_max < w_min": dict(w_max=-2.0), "nv 0": dict(nv=0),
              "nv 65": dict(nv=65), "nw 0": dict(nw=0), "nw 65": dict(nw=65), "sim 0": dict(sim_time_s=0.0), "sim < 0": dict(sim_time_s=-1.0),
              "sim nan": dict(sim_time_s=float("nan")), "steps 0": dict(steps=0), "steps 65": dict(steps=65), "lethal 0": dict(lethal_cost=0),
              "lethal 256": dict(lethal_cost=256), "centre 0": dict(centre_lethal_cost=0), "centre 256": dict(centre_lethal_cost=256),
              "unknown -1": dict(unknown_cost=-1), "unknown 253": dict(unknown_cost=253), "flags 2": dict(flags=2), "w_goal -1": dict(w_goal=-1),
              "w_goal 32768": dict(w_goal=32768), "w_occ -1": dict(w_occ=-1), "w_occ 32768": dict(w_occ=32768), "both weights 0": dict(w_goal=0, w_occ=0),
              "an arc too long": dict(v_max=500.0, sim_time_s=30.0), "too many turns": dict(w_max=3.0e6, sim_time_s=10.0)}


def test_every_refusal_on_both_sides():
    lib = api.load_library()
    for name, kw in BAD_PARAMS.items():
        p = dataclasses.replace(P0, **kw)
        with pytest.raises(ValueError):
            rollout.tables(p, FP0)
        with pytest.raises(api.StereoNetError):
            api.rollout_tables(p, FP0)
        prm = api.rollout_params(p)
        assert lib.sn_rollout_tables(C.byref(prm), FP0.ctypes.data, len(FP0), None, None) == -1, name
    nan_fp, far_fp, many = FP0.copy(), FP0.copy(), np.zeros((65, 2), np.float32)
    nan_fp[2, 0], far_fp[1] = np.inf, (0.0, -500.0)
    for fp in (nan_fp, far_fp, many):
        with pytest.raises(ValueError):
            rollout.tables(P0, fp)
        with pytest.raises(api.StereoNetError):
            api.rollout_tables(P0, fp)
    prm = api.rollout_params(P0)
    assert lib.sn_rollout_tables(None, FP0.ctypes.data, len(FP0), None, None) == -1
    assert lib.sn_rollout_tables(C.byref(prm), None, 3, None, None) == -1 and lib.sn_rollout_tables(C.byref(prm), None, 0, None, None) == 0
    assert lib.sn_rollout_tables(C.byref(prm), FP0.ctypes.data, -1, None, None) == -1
    # the bounds themselves pass: a reach of exactly 2^21 / 256 = 8192 cells
    edge = dataclasses.replace(P0, cell_m=1.0, v_min=0.0, v_max=8192.0, nv=2, w_min=0.0, w_max=0.0, nw=1, sim_time_s=1.0, steps=1)
    assert api.rollout_tables(edge, ())[0][1, 1, 0] == 1 << 21 and rollout.tables(edge, ())[0][1, 1, 0] == 1 << 21
    for fp in ([(0.01, 0.0)], ()):
        over = dataclasses.replace(edge, v_max=8192.0 if len(fp) else 8192.01)
        with pytest.raises(ValueError):
            rollout.tables(over, fp)
        with pytest.raises(api.StereoNetError):
            api.rollout_tables(over, fp)
    # the velocity of a sample that is not there
    for s in (-1, P0.nv * P0.nw):
        with pytest.raises(ValueError):
            rollout.velocity(P0, s)
        with pytest.raises(api.StereoNetError):
            api.rollout_velocity(P0, s)
    # poses
    for cell, ox, pose in ((0.0, 0.0, (0, 0, 0)), (float("nan"), 0.0, (0, 0, 0)), (0.05, float("inf"), (0, 0, 0)), (0.05, 0.0, (float("nan"), 0, 0)),
                           (0.05, 0.0, (0, 0, float("inf"))), (0.05, 0.0, (0, 0, 2.0e6)), (0.05, 0.0, (0, 0.05 * 2 ** 22 + 1, 0)), (0.05, 3.0e5, (0, 0, 0))):
        with pytest.raises(ValueError):
            rollout.pose_q(cell, ox, 0.0, pose)
        with pytest.raises(api.StereoNetError):
            api.rollout_pose_q(cell, ox, 0.0, pose)
    assert abs(int(api.rollout_pose_q(1.0, 0.0, 0.0, (2.0 ** 22, 0, 0))[0])) == 1 << 30      # the bound itself
    # the twin refuses what is not a call
    centres, offsets = api.rollout_tables(P0, FP0)
    cost, pot = np.zeros((2, 5, 6), np.uint8), np.zeros((2, 5, 6), np.uint32)
    q = api.rollout_pose_q(0.05, 0, 0, [(0.1, 0.1, 0.0)] * 2)
    with pytest.raises(ValueError):
        rollout.reference(cost, pot, q[:1], None, P0, centres, offsets)
    with pytest.raises(ValueError):
        rollout.reference(cost, pot, q, None, P0, centres[:-1], offsets)
    with pytest.raises(ValueError):
        rollout.reference(cost, pot, q, np.zeros((1, 4)), P0, centres, offsets)
    with pytest.raises(ValueError):
        rollout.reference(cost, pot, q.astype(np.int64) * 4, None, P0, centres, offsets)
    with pytest.raises(ValueError):
        rollout.reference(cost, pot, q, None, dataclasses.replace(P0, flags=2), centres, offsets)


def test_window_from_velocity():
    p = dataclasses.replace(P0, v_min=0.0, v_max=0.4, nv=5, w_min=-1.0, w_max=1.0, nw=5)      # v: 0, .1, .2, .3, .4; w: -1, -.5, 0, .5, 1
    win = rollout.window_from_velocity
    assert win(p, 0.2, 0.0, 1.0, 5.0, 0.11).tolist() == [1, 3, 1, 3] and win(p, 0.2, 0.0, 1.0, 5.0, 0.11).dtype == np.int32
    assert win(p, 0.2, 0.0, 100.0, 100.0, 1.0).tolist() == [0, 4, 0, 4]                       # everything in reach: clamped to the lattice
    assert win(p, 0.0, -1.0, 1.0, 5.0, 0.11).tolist() == [0, 1, 0, 1]                         # at the lattice's corner
    assert win(p, 0.24, 0.3, 1.0, 1.0, 0.0).tolist() == [2, 2, 3, 3]                          # dt = 0: the nearest sample on each axis
    assert win(p, 0.25, 0.25, 0.0, 0.0, 1.0).tolist()[2:] == [2, 2]                           # a tie goes to the lower sample
    assert win(p, 9.0, -9.0, 1.0, 1.0, 0.1).tolist() == [4, 4, 0, 0]                          # far outside the lattice: its nearest end
    assert win(p, 0.15, 0.0, 0.2, 1.0, 0.1).tolist()[:2] == [1, 1] or win(p, 0.15, 0.0, 0.2, 1.0, 0.1).tolist()[:2] == [2, 2]
    one = dataclasses.replace(p, nv=1, nw=1)
    assert win(one, 0.3, 0.7, 1.0, 1.0, 0.1).tolist() == [0, 0, 0, 0]
    for bad in ((float("nan"), 0, 1, 1, 1), (0, 0, -1, 1, 1), (0, 0, 1, -1, 1), (0, 0, 1, 1, -0.1), (0, float("inf"), 1, 1, 1)):
        with pytest.raises(ValueError):
            win(p, *bad)
    with pytest.raises(ValueError):
        win(dataclasses.replace(p, nv=0), 0, 0, 1, 1, 1)
    # the window is what sn_rollout takes: every sample outside it is out of window and nothing else
    centres, offsets = api.rollout_tables(p, ())
    w4 = win(p, 0.2, 0.0, 1.0, 5.0, 0.11)
    s, b, _ = rollout.reference(np.zeros((40, 40), np.uint8), np.zeros((40, 40), np.uint32), api.rollout_pose_q(0.05, 0, 0, (1.0, 1.0, 0.3)), w4, p,
                                centres, offsets)
    assert b[0, 4:].tolist() == [9, 0, 0, 16]


def test_rectangle_footprint():
    fp = rollout.rectangle_footprint(0.6, 0.4, 0.1)
    assert fp.dtype == np.float32 and fp.shape == (20, 2) and len({tuple(x) for x in fp.tolist()}) == 20
    assert np.allclose(fp[:, 0].max(), 0.3) and np.allclose(fp[:, 0].min(), -0.3) and np.allclose(fp[:, 1].max(), 0.2) and np.allclose(fp[:, 1].min(), -0.2)
    assert np.all(np.isclose(np.abs(fp[:, 0]), 0.3) | np.isclose(np.abs(fp[:, 1]), 0.2))                  # on the outline
    gaps = np.linalg.norm(fp - np.roll(fp, -1, 0), axis=1)
    assert gaps.max() <= 0.1 + 1e-6
    assert rollout.rectangle_footprint(0.6, 0.4, 0.05).shape == (40, 2) and rollout.rectangle_footprint(0.6, 0.4, 10.0).shape == (4, 2)
    assert rollout.rectangle_footprint(0.8, 0.8, 0.05).shape == (64, 2)
    for bad in ((0.6, 0.4, 0.025), (0.0, 0.4, 0.1), (0.6, -1.0, 0.1), (0.6, 0.4, 0.0), (float("nan"), 0.4, 0.1)):
        with pytest.raises(ValueError):
            rollout.rectangle_footprint(*bad)


def test_header_constants_equal_the_modules():
    text = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
    defs = {m.group(1): m.group(2) for m in re.finditer(r"#define (SN_(?:ROLLOUT|NAV)_[A-Z_]+)\s+(\S+)", text)}
    want = {"SN_ROLLOUT_MAX_STEPS": rollout.MAX_STEPS, "SN_ROLLOUT_MAX_POINTS": rollout.MAX_POINTS, "SN_ROLLOUT_MAX_SIDE": rollout.MAX_SIDE,
            "SN_ROLLOUT_UNKNOWN_OK": rollout.UNKNOWN_OK, "SN_ROLLOUT_NO_VALID": rollout.NO_VALID, "SN_ROLLOUT_VALID": VALID,
            "SN_ROLLOUT_OUT_OF_WINDOW": OUT_OF_WINDOW, "SN_ROLLOUT_COLLISION": COLLISION, "SN_ROLLOUT_NO_ROUTE": NO_ROUTE}
    for k, v in want.items():
        assert int(defs[k], 0) == v, k
    assert int(defs["SN_NAV_INF"].rstrip("u"), 0) == INF
    src = open(os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "sn_rollout.hpp")).read()
    assert int(re.search(r"kRoWaves = (\d+)", src).group(1)) == rollout.GROUP
    assert int(re.search(r"kRoBestThreads = (\d+)", src).group(1)) == rollout.BEST_THREADS
    assert C.sizeof(api.SnRolloutParams) == 15 * 4 and [f[0] for f in api.SnRolloutParams._fields_] == \
        ["cell_m", "v_min", "v_max", "nv", "w_min", "w_max", "nw", "sim_time_s", "steps", "lethal_cost", "centre_lethal_cost", "unknown_cost",
         "flags", "w_goal", "w_occ"]
    assert len(rollout.REASONS) == 4 and rollout.BEST[0] == "flags" and len(rollout.BEST) == 8


def test_parameter_file_round_trips(tmp_path):
    p = dataclasses.replace(P0, footprint=tuple(map(tuple, FP0.astype(np.float64).tolist())), pose=(1.25, -0.5, 0.3), acc=(0.5, 2.0, 0.25))
    path = str(tmp_path / "r.txt")
    rollout.save_params(path, p)
    assert rollout.load_params(path) == p
    rollout.save_params(path, P0)
    assert rollout.load_params(path) == P0 and rollout.load_params(path).pose is None
    for text in ("nv 3\nnv 4\n", "bogus 1\n", "nv 1.5\n", "pose 1 2\n", "acc 1 2\n", "point 1\n", "cell_m x\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(ValueError):
            rollout.load_params(path)
    with open(path, "w") as f:
        f.write("# only a comment\nnv 3  # three\npoint 0.1 0.2\npoint -0.1 0.2\n")
    got = rollout.load_params(path)
    assert got.nv == 3 and got.footprint == ((0.1, 0.2), (-0.1, 0.2)) and got.nw == RolloutParams().nw


def test_the_benchs_host_loop_equals_the_twin(tmp_path):
    """rollout_harness --bench, the one-thread C++ loop scripts/bench_rollout.py times the kernel against, picks the twin's sample"""
    import json
    import subprocess
    compat = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
    subprocess.check_call(["make", "-C", compat, "-s", "build/rollout_harness"])
    rng = np.random.default_rng(17)
    kinds = set()
    for flags, dense in ((0, 0.004), (rollout.UNKNOWN_OK, 0.004), (0, 0.5)):
        p = dataclasses.replace(P0, flags=flags)
        centres, offsets = api.rollout_tables(p, FP0)
        cost, pot = _maps(rng, 1, 33, 47, dense)
        q = api.rollout_pose_q(p.cell_m, 0.0, 0.0, [(1.1, 0.8, 0.4)])
        _, best, _ = rollout.reference(cost, pot, q, None, p, centres, offsets)
        files = []
        for name, a in (("cost", cost[0]), ("pot", pot[0]), ("centres", centres), ("offsets", offsets)):
            files.append(str(tmp_path / f"{name}.bin"))
            np.ascontiguousarray(a).tofile(files[-1])
        args = [47, 33, p.nv, p.nw, p.steps, len(FP0), *q[0, :4].tolist(), p.lethal_cost, p.centre_lethal_cost, p.unknown_cost if flags else -1,
                p.w_goal, p.w_occ, 2]
        r = subprocess.run([os.path.join(compat, "build", "rollout_harness"), "--bench"] + files + [str(v) for v in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = json.loads(r.stdout)
        none = bool(best[0, 0] & rollout.NO_VALID)
        assert got["s_best"] == (-1 if none else int(best[0, 1])) and got["score"] == (-1 if none else int(best[0, 2]) | int(best[0, 3]) << 32)
        assert [got["valid"], got["collided"], got["no_route"]] == best[0, 4:7].tolist() and got["loop_us"] > 0
        kinds.add(none)
    assert kinds == {False, True}
    assert subprocess.run([os.path.join(compat, "build", "rollout_harness")], capture_output=True).returncode == 2
