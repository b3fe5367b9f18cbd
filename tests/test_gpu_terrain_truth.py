"""The elevation map and its traversability verdict against float64 terrain geometry, on the kernels: the scenes, the truth and
the checks of tests/test_terrain_truth.py applied to what sn_elevation_push (and sn_inflate_grid, sn_navfn behind it) wrote on the
MI355X, in host mode with the clip pushed at once and frame by frame, in device mode on one stream (the maps uploaded once,
nothing crossing to the host between the stages, every output between guard bytes in buffers filled with 0x5a), and with four
scenes as one batch of four streams.  The kernels' bytes also equal the twin's, which says on which side a physical failure
lies.  No forward pass: the maps are the truth's."""
import dataclasses

import numpy as np
import pytest

import terrain_truth as tt
import test_terrain_truth as T
from hobot_stereonet_amd import api, navfn

W, H, D = tt.W, tt.H, 48
MAX_BATCH = 8
GUARD = 16
TWIN_KEYS = ("trav", "hi", "lo", "rise", "stats", "q")


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=MAX_BATCH) as e:
        yield e


class Engine:
    """host mode: the calls of the engine in the places of the twins"""

    def __init__(self, eng):
        self.eng = eng

    def elevation(self, p, poses, raws):
        with self.eng.elevation(p) as ev:
            return ev.push(poses, raws, T.CAM)

    def inflate(self, grid, ip):
        return self.eng.inflate(grid, ip)[0]

    def navfn(self, cost, goals, starts, nav):
        return self.eng.navfn(cost, goals, starts, nav)[:3]


def _differing(R, want, keys=TWIN_KEYS):
    return [k for k in keys if np.asarray(R[k]).tobytes() != np.asarray(want[k]).tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tt.SCENES))
def test_host_mode_against_the_truth(eng, name):
    t, want = tt.SCENES[name], T.twin_map(name)
    print(f"terrain_truth {name} | mode | host")
    R = T.run_map(t, Engine(eng))
    bad = T.failures(name, R)
    assert not bad, bad
    assert not _differing(R, want), _differing(R, want)
    if t.goal is not None and (t.ramp is not None or t.pitch):
        T.check_plan(name, R, Engine(eng))
    # the clip once more frame by frame: the same bytes as the one push
    with eng.elevation(R["p"]) as ev:
        for k, pose in enumerate(t.poses):
            one = ev.push([pose], R["raws"][k], T.CAM)
            assert all(one[i].tobytes() == R[key][k:k + 1].tobytes() for i, key in enumerate(TWIN_KEYS)), k


@pytest.mark.gpu
def test_the_mirrored_world_on_the_device(eng):
    for name in ("kerb", "flat and wall"):
        a, b = (T.run_map(tt.SCENES[n], Engine(eng)) for n in (name, name + " mirrored"))
        T.check_mirror(name, name + " mirrored", a, b)


def _buffer(torch, nbytes):
    return torch.full((nbytes + 2 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")


def _read(buf, nbytes, dtype, shape, what):
    o = buf.cpu().numpy()
    assert np.all(o[:GUARD] == 0x5a) and np.all(o[GUARD + nbytes:] == 0x5a), f"guard bytes around {what}"
    return o[GUARD:GUARD + nbytes].view(dtype).reshape(shape).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ramp", "drop mirrored"])
def test_device_mode_on_one_stream_against_the_truth(eng, name):
    """elevation -> inflation -> navigation function on one stream of the caller's"""
    import torch
    t, want = tt.SCENES[name], T.twin_map(name)
    print(f"terrain_truth {name} | mode | device")
    poses = np.asarray(t.poses, np.float64)
    n, (mw, mh) = len(poses), t.window
    p = T.params(t)
    nav = dataclasses.replace(T.NAV_OK if t.ramp is not None else T.NAV_STRICT, max_rounds=4 * (mw + mh))
    c = n * mw * mh
    spec = dict(trav=(c, np.int8, (n, mh, mw)), hi=(2 * c, np.int16, (n, mh, mw)), lo=(2 * c, np.int16, (n, mh, mw)), rise=(2 * c, np.uint16, (n, mh, mw)),
                stats=(16 * n, np.uint32, (n, 4)), cost=(mw * mh, np.uint8, (mh, mw)), pot=(4 * mw * mh, np.uint32, (mh, mw)),
                path=(8 * nav.max_path, np.int32, (nav.max_path, 2)), nav_stats=(20, np.uint32, (5,)))
    bufs = {k: _buffer(torch, v[0]) for k, v in spec.items()}
    ptr = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    with eng.elevation(p) as ev:
        q_host = ev.pose_q(poses)
        origin = (int(q_host[-1][4]), int(q_host[-1][5]))
        assert origin == T.truth(name)["origin"]
        (gx, gy), (sx, sy) = T.world_cell(t.goal), T.world_cell(poses[-1])
        goal, start = (gx - origin[0], gy - origin[1]), (sx - origin[0], sy - origin[1])
        d_raw = torch.from_numpy(np.stack([tt.render(t, x) for x in poses])).cuda()      # uploaded once
        d_goal, d_start = (torch.from_numpy(np.array(a, np.int32).reshape(1, -1)).cuda() for a in (goal, start))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = side.cuda_stream
        q = ev.push_device(n, poses, d_raw.data_ptr(), T.CAM, trav_ptr=ptr["trav"], hi_ptr=ptr["hi"], lo_ptr=ptr["lo"], rise_ptr=ptr["rise"],
                           stats_ptr=ptr["stats"], stream=s)
        eng.inflate_device(1, ptr["trav"] + (n - 1) * mw * mh, mw, mh, T.IP, cost_ptr=ptr["cost"], stream=s)
        eng.navfn_device(1, ptr["cost"], mw, mh, d_goal.data_ptr(), d_start.data_ptr(), nav, potential_ptr=ptr["pot"], path_ptr=ptr["path"],
                         stats_ptr=ptr["nav_stats"], stream=s)
        torch.cuda.synchronize()
    assert np.array_equal(q, q_host)
    R = {k: _read(bufs[k], *spec[k], k) for k in spec}
    R.update(q=q, origin=origin, p=p)
    bad = T.failures(name, R)
    assert not bad, bad
    assert not _differing(R, want), _differing(R, want)
    assert not R["nav_stats"][0] & navfn.UNCONVERGED, R["nav_stats"].tolist()
    length = int(R["nav_stats"][2])
    if t.ramp is not None:
        cells = R["path"][:length].astype(np.int64)
        on_ramp = ((cells[:, 0] + origin[0] + 0.5) * T.CELL > t.ramp[0]) & ((cells[:, 0] + origin[0] + 0.5) * T.CELL < t.ramp[1])
        print(f"terrain_truth {name} | plan | device: flags {int(R['nav_stats'][0])}, {length} cells, {int(on_ramp.sum())} of them on the ramp")
        assert R["nav_stats"][0] == 0 and tuple(cells[0]) == start and tuple(cells[-1]) == goal and on_ramp.sum() >= 10
    else:
        print(f"terrain_truth {name} | plan | device: flags {int(R['nav_stats'][0])} (start unreachable = {navfn.START_UNREACHABLE})")
        assert R["nav_stats"][0] == navfn.START_UNREACHABLE and R["cost"][goal[1], goal[0]] < 253 and R["cost"][start[1], start[0]] < 253


@pytest.mark.gpu
def test_four_scenes_as_one_batch_of_streams(eng):
    """the four scenes as four streams of one object, a frame of each per push: every row equals what the scene gave alone"""
    names = [t.name for t in tt.BASE]
    scenes, want = [tt.SCENES[n] for n in names], [T.twin_map(n) for n in names]
    frames = len(scenes[0].poses)
    # one object needs one mount: the level scenes share theirs, the pitched one gets its own through `mounts`
    p = T.params(scenes[0])
    mounts = np.asarray([tt.mount(s) for s in scenes], np.float32)
    outs = []
    with eng.elevation(p, streams=4) as ev:
        for k in range(frames):
            raws = np.stack([tt.render(s, s.poses[k]) for s in scenes])
            outs.append(ev.push([s.poses[k] for s in scenes], raws, T.CAM, mounts=mounts, stream_of=[0, 1, 2, 3]))
    for i, name in enumerate(names):
        print(f"terrain_truth {name} | mode | row {i} of a batch of 4")
        R = {key: np.stack([o[j][i] for o in outs]) for j, key in enumerate(TWIN_KEYS)}
        R.update(origin=(int(R["q"][-1][4]), int(R["q"][-1][5])), p=p)
        bad = T.failures(name, R)
        assert not bad, (name, bad)
        assert not _differing(R, want[i]), (name, _differing(R, want[i]))
