"""The chain from the map to the command against float64 scene geometry, on the kernels: the scenes, the truth and the checks of
tests/test_chain_truth.py applied to what sn_ground_from_raw, sn_obstacles_from_raw, sn_costmap_push, sn_inflate_grid, sn_navfn
and sn_rollout wrote on the MI355X, in host mode, in device mode on one stream (the map uploaded once, nothing crossing to the
host between the stages, every output between guard bytes in buffers filled with 0x5a), with the clip pushed at once and frame by
frame, and with three scenes as one batch.  The kernels' bytes also equal the twin chain's, which says on which side a physical
failure lies.  No forward pass: the maps are the truth's."""
import dataclasses

import numpy as np
import pytest

import scene_truth as st
import test_chain_truth as ct
from hobot_stereonet_amd import api, ground, navfn

W, H, D = st.W, st.H, 48
MAX_BATCH = 12
GUARD = 16
LEVEL_SCENES = ("free end", "free end mirrored", "gap and box")      # one window size: a batch of 3
TWIN_KEYS = ("occ", "ranges", "grid", "logodds", "q", "cost", "pot", "path", "nav_stats", "samples", "best", "traj")


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


class Engine:
    """host mode: the calls of the engine in the places of the twins"""

    def __init__(self, eng):
        self.eng, self.rounds = eng, None

    def mounts(self, raws):
        return np.ascontiguousarray(self.eng.ground(raws, ct.CAM, ct.GP, labels=False)[0]["base_from_cam"], np.float32)

    def obstacles(self, raws, op, mounts):
        occ, _, _, ranges, _ = self.eng.obstacles(raws, ct.CAM, op, mounts=mounts)
        return occ, ranges

    def costmap(self, cp, op, poses, occ, ranges):
        with self.eng.costmap(op, cp) as cm:
            grid, logodds, _, q = cm.push(poses, occ, ranges)
        return grid, logodds, q

    def inflate(self, grid, ip):
        return self.eng.inflate(grid, ip)[0]

    def navfn(self, cost, goals, starts, nav):
        pot, path, stats, self.rounds = self.eng.navfn(cost, goals, starts, nav)
        return pot, path, stats

    def rollout(self, cost, pot, q5, rp, fp):
        return self.eng.rollout(cost, pot, q5, rp, fp)


def _differing(R, want, keys=TWIN_KEYS):
    """the outputs whose bytes differ from the twin chain's"""
    return [k for k in keys if np.asarray(R[k]).tobytes() != np.asarray(want[k]).tobytes()]


def _checks(name):
    return dict(ct.CHECKS, scroll=ct.check_scroll) if st.SCENES[name].window != (100, 100) else ct.CHECKS


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(st.SCENES))
def test_host_mode_against_the_truth(eng, name):
    scene, want = st.SCENES[name], ct.twin_chain(name)
    print(f"chain_truth {name} | mode | host")
    be = Engine(eng)
    R = ct.run_chain(scene, be)
    bad = ct.failures(name, R, _checks(name))
    assert not bad, bad
    assert scene.fitted_mount == (R["mounts"] is not None) and (R["mounts"] is None or R["mounts"].tobytes() == want["mounts"].tobytes())
    assert not _differing(R, want), _differing(R, want)
    # the clip once more frame by frame: the same bytes as the one push
    cp = ct.costmap_params(scene)
    with eng.costmap(ct.OP, cp) as cm:
        for k, pose in enumerate(scene.poses):
            grid, logodds, _, q = cm.push([pose], R["occ"][k:k + 1], R["ranges"][k:k + 1])
            assert grid.tobytes() == R["grid"][k].tobytes() and logodds.tobytes() == R["logodds"][k].tobytes() and np.array_equal(q[0], R["q"][k]), k


@pytest.mark.gpu
def test_the_mirrored_world_on_the_device(eng):
    for name in ("free end", "corridor"):
        a, b = (ct.run_chain(st.SCENES[n], Engine(eng)) for n in (name, name + " mirrored"))
        ct.check_mirror(name, name + " mirrored", a, b)


def _buffer(torch, nbytes):
    return torch.full((nbytes + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")


def _read(buf, nbytes, dtype, shape, what):
    o = buf.cpu().numpy()
    assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + nbytes:] == 0x5a), f"guard bytes around {what}"
    return o[GUARD:GUARD + nbytes].view(dtype).reshape(shape).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(st.SCENES))
def test_device_mode_on_one_stream_against_the_truth(eng, name):
    import torch
    scene, want = st.SCENES[name], ct.twin_chain(name)
    print(f"chain_truth {name} | mode | device")
    poses = np.asarray(scene.poses, np.float64)
    n, (mw, mh) = len(poses), scene.window
    op, cp, rp = ct.OP, ct.costmap_params(scene), ct.RP
    # how many rounds the field takes, from a host-mode call that runs until nothing changes; the device call gets twice that
    host = Engine(eng)
    host.navfn(want["cost"][None], [want["goal"]], [want["start"]], ct.NAV)
    nav = dataclasses.replace(ct.NAV, max_rounds=2 * host.rounds)
    assert host.rounds >= 1
    S, T1 = rp.nv * rp.nw, rp.steps + 1
    spec = dict(occ=(n * op.gw * op.gh, np.int8, (n, op.gh, op.gw)), ranges=(4 * n * op.beams, np.float32, (n, op.beams)),
                grid=(n * mw * mh, np.int8, (n, mh, mw)), logodds=(2 * n * mw * mh, np.int16, (n, mh, mw)), cost=(mw * mh, np.uint8, (mh, mw)),
                pot=(4 * mw * mh, np.uint32, (mh, mw)), path=(8 * nav.max_path, np.int32, (nav.max_path, 2)), nav_stats=(20, np.uint32, (5,)),
                samples=(8 * S, np.uint32, (S, 2)), best=(32, np.uint32, (8,)), traj=(12 * T1, np.int32, (T1, 3)))
    bufs = {k: _buffer(torch, v[0]) for k, v in spec.items()}
    ptr = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    records = _buffer(torch, n * 4 * ground.RECORD_FLOATS) if scene.fitted_mount else None
    with eng.costmap(op, cp) as cm:
        q_host = cm.pose_q(poses)                                                # the quantised poses are the host's: known before the chain
        origin = (int(q_host[-1][4]), int(q_host[-1][5]))
        assert origin == ct.truth(name)["origins"][-1]
        (gx, gy), (sx, sy) = ct.world_cell(scene.goal), ct.world_cell(poses[-1])
        goal, start = (gx - origin[0], gy - origin[1]), (sx - origin[0], sy - origin[1])
        q5 = api.rollout_pose_q(ct.CELL, origin[0] * ct.CELL, origin[1] * ct.CELL, poses[-1:])
        d_raw = torch.from_numpy(np.stack([st.render(scene, p) for p in poses])).cuda()      # uploaded once
        d_goal, d_start, d_q5 = (torch.from_numpy(np.array(a, np.int32).reshape(1, -1)).cuda() for a in (goal, start, q5))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = side.cuda_stream
        mounts = {}
        if scene.fitted_mount:
            eng.ground_device(n, d_raw.data_ptr(), ct.CAM, ct.GP, ground_ptr=records.data_ptr() + GUARD, stream=s)
            mounts = dict(mounts_ptr=records.data_ptr() + GUARD + 4 * ground.MOUNT_OFFSET_FLOATS, mount_stride=ground.RECORD_FLOATS)
        eng.obstacles_device(n, d_raw.data_ptr(), ct.CAM, op, occ_ptr=ptr["occ"], ranges_ptr=ptr["ranges"], stream=s, **mounts)
        q = cm.push_device(n, poses, occ_ptr=ptr["occ"], ranges_ptr=ptr["ranges"], grid_ptr=ptr["grid"], logodds_ptr=ptr["logodds"], stream=s)
        eng.inflate_device(1, ptr["grid"] + (n - 1) * mw * mh, mw, mh, ct.IP, cost_ptr=ptr["cost"], stream=s)
        assert eng.navfn_device(1, ptr["cost"], mw, mh, d_goal.data_ptr(), d_start.data_ptr(), nav, potential_ptr=ptr["pot"], path_ptr=ptr["path"],
                                stats_ptr=ptr["nav_stats"], stream=s) == -1
        eng.rollout_device(1, ptr["cost"], ptr["pot"], mw, mh, d_q5.data_ptr(), rp, ct.FOOTPRINT, 0, ptr["samples"], ptr["best"], ptr["traj"], stream=s)
        torch.cuda.synchronize()
    assert np.array_equal(q, q_host)
    R = {k: _read(bufs[k], *spec[k], k) for k in spec}
    R.update(q=q, origin=origin, goal=goal, start=start, q5=q5, arc_sign=1.0)
    if scene.fitted_mount:
        rec = _read(records, n * 4 * ground.RECORD_FLOATS, np.uint8, (-1,), "the ground records").view(ground.RECORD)
        assert np.ascontiguousarray(rec["base_from_cam"]).tobytes() == want["mounts"].tobytes()
    assert not R["nav_stats"][0] & navfn.UNCONVERGED, R["nav_stats"].tolist()
    length = int(R["nav_stats"][2])
    assert np.all(R["path"][length:] == 0x5a5a5a5a), "entries past the path's length are not written"
    R["path"][length:] = -1                                                     # as host mode and the twin give them
    bad = ct.failures(name, R, _checks(name))
    assert not bad, bad
    assert not _differing(R, want), _differing(R, want)


@pytest.mark.gpu
def test_three_scenes_as_one_batch(eng):
    """The mirrored pair and a further scene as one batch of 3 through every stage: three maps per obstacle call, three streams of
    one costmap fed a frame each per push, three grids per inflation, field and rollout.  Every row equals what the scene gave
    alone, so the batch satisfies the same assertions; they are run on its rows all the same."""
    scenes = [st.SCENES[n] for n in LEVEL_SCENES]
    want = [ct.twin_chain(n) for n in LEVEL_SCENES]
    frames = len(scenes[0].poses)
    assert all(len(s.poses) == frames and s.window == scenes[0].window for s in scenes)
    cp = ct.costmap_params(scenes[0])
    occs, rngs, grids, lods, qs = [], [], [], [], []
    with eng.costmap(ct.OP, cp, streams=3) as cm:
        for k in range(frames):
            raws = np.stack([st.render(s, s.poses[k]) for s in scenes])
            occ, _, _, ranges, _ = eng.obstacles(raws, ct.CAM, ct.OP)
            grid, logodds, _, q = cm.push([s.poses[k] for s in scenes], occ, ranges, stream_of=[0, 1, 2])
            for acc, a in zip((occs, rngs, grids, lods, qs), (occ, ranges, grid, logodds, q)):
                acc.append(a)
    cost = eng.inflate(grids[-1], ct.IP)[0]
    pot, path, stats, _ = eng.navfn(cost, [w["goal"] for w in want], [w["start"] for w in want], ct.NAV)
    q5 = np.concatenate([w["q5"] for w in want])
    samples, best, traj = eng.rollout(cost, pot, q5, ct.RP, ct.FOOTPRINT)
    for i, name in enumerate(LEVEL_SCENES):
        print(f"chain_truth {name} | mode | row {i} of a batch of 3")
        R = dict(occ=np.stack([a[i] for a in occs]), ranges=np.stack([a[i] for a in rngs]), grid=np.stack([a[i] for a in grids]),
                 logodds=np.stack([a[i] for a in lods]), q=np.stack([a[i] for a in qs]), cost=cost[i], pot=pot[i], path=path[i], nav_stats=stats[i],
                 samples=samples[i], best=best[i], traj=traj[i], origin=(int(qs[-1][i][4]), int(qs[-1][i][5])), arc_sign=1.0)
        bad = ct.failures(name, R)
        assert not bad, (name, bad)
        assert not _differing(R, want[i]), (name, _differing(R, want[i]))
