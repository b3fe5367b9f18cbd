"""The node's published messages against float64 scene geometry, on the real node: csrc/compat/test/scene_harness.cpp hands
StereonetNode::PostProcess the analytic scenes' maps (tests/golden/scene_truth.py) frame by frame with the true poses and the
goal, and records every message whole; tests/golden/node_messages.py decodes them by the ROS conventions alone and
tests/test_node_truth.py's checks hold them to the truth.  No forward pass: the model file gives the engine its geometry.

A failure of a truth check with the byte diagnostic at 0 lies in the node's glue (stereonet_node.cpp); with bytes that differ
from the api chain of tests/test_gpu_chain_truth.py on the same maps, in a stage or in what the node hands it.

One harness run per scene, each a child process with a time limit; after a run that ended on a signal, an abort, a time limit or
a log naming an illegal memory access, no further harness is started in the session and the remaining cases fail with that reason.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import node_messages as nm
import scene_truth as st
import test_chain_truth as ct
import test_node_truth as nt
from test_gpu_chain_truth import Engine
from hobot_stereonet_amd import api, costmap, ground, inflate, navfn, obstacles, rollout

W, H, D = st.W, st.H, 48
HARNESS_TIMEOUT_S = 300                      # as the other node tests give a harness of this geometry
CAMERA_ENV = f"{nt.CAM.fx!r},{nt.CAM.fy!r},{nt.CAM.cx!r},{nt.CAM.cy!r},{nt.CAM.baseline_mm!r}"


class Harness:
    """runs scene_harness once per key and keeps what it recorded; after a run that took the GPU down with it, runs nothing more"""

    def __init__(self, model, tmp):
        self.model, self.tmp, self.done, self.dead = model, tmp, {}, None

    def run(self, key, scene, poses, goal, raws, window):
        if key in self.done:
            return self.done[key]
        assert self.dead is None, f"no further harness run in this session: {self.dead}"
        d = self.tmp / key.replace(" ", "_")
        d.mkdir()
        P = nt.node_params(scene)
        obstacles.save_params(str(d / "ob.txt"), P.op)
        costmap.save_params(str(d / "cm.txt"), dataclasses.replace(P.cp, mw=window[0], mh=window[1]))
        inflate.save_params(str(d / "in.txt"), P.ip)
        navfn.save_params(str(d / "plan.txt"), P.nav)
        rollout.save_params(str(d / "roll.txt"), P.rp)
        np.ascontiguousarray(raws, np.int32).tofile(str(d / "raws.bin"))
        np.savetxt(str(d / "poses.txt"), np.asarray(poses, np.float64).reshape(-1, 3), fmt="%.17g")
        env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", STEREONET_CAMERA=CAMERA_ENV,
                   STEREONET_POINTCLOUD="organised", STEREONET_POINTCLOUD_Z=f"{nt.CLOUD_Z[0]!r},{nt.CLOUD_Z[1]!r}", STEREONET_OBSTACLES=str(d / "ob.txt"),
                   STEREONET_COSTMAP=str(d / "cm.txt"), STEREONET_INFLATE=str(d / "in.txt"), STEREONET_PLAN=str(d / "plan.txt"),
                   STEREONET_ROLLOUT=str(d / "roll.txt"))
        if scene.fitted_mount:
            ground.save_params(str(d / "gr.txt"), P.gp)
            env["STEREONET_GROUND"] = str(d / "gr.txt")
        args = [os.path.join(nt.COMPAT, "build", "scene_harness"), self.model, str(W), str(H), str(d / "raws.bin"), str(len(poses)), str(d / "poses.txt"),
                repr(float(goal[0])), repr(float(goal[1])), str(d / "m")]
        try:
            r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=HARNESS_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            self.dead = f"the run of {key!r} was killed at its time limit of {HARNESS_TIMEOUT_S} s"
            raise AssertionError(self.dead)
        log = r.stdout + r.stderr
        if r.returncode < 0 or r.returncode in (4, 134, 139) or "illegal memory access" in log:
            self.dead = f"the run of {key!r} ended with {r.returncode}: {log[-400:]}"
        assert r.returncode == 0 and self.dead is None, (r.returncode, log[-2000:])
        M = nm.load_recording(r.stdout, str(d / "m"))
        per_frame = ["cloud", "grid", "scan", "costmap", "inflated", "plan", "cmd", "local_plan"]
        assert M["order"] == per_frame * len(poses), M["order"][:16]
        for kind in ("/stereonet_obstacle_grid", "/stereonet_scan", "/stereonet_costmap", "/stereonet_inflated_grid", "/stereonet_plan", "/stereonet_cmd_vel",
                     "/stereonet_pointcloud2") + (("ground:",) if scene.fitted_mount else ()):
            assert kind in log, (kind, log[-2000:])
        self.done[key] = M
        return M

    def scene(self, name):
        scene = st.SCENES[name]
        raws = np.stack([st.render(scene, p) for p in scene.poses])
        return self.run(name, scene, scene.poses, scene.goal, raws, scene.window)


@pytest.fixture(scope="module")
def harness(model_factory, tmp_path_factory):
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", nt.COMPAT, "-s", "build/scene_harness"])
    return Harness(model_factory(W, H, D), tmp_path_factory.mktemp("node_truth"))


@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(W, H, D), max_batch=12) as e:
        yield e


def differing_bytes(M, R, rp):
    """how many bytes of the node's grids, scans, path cells and best sample differ from an api chain's on the same maps"""
    out = {}

    def count(a, b):
        a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
        return int(abs(a.size - b.size) + np.count_nonzero(a[:min(a.size, b.size)] != b[:min(a.size, b.size)]))
    n = len(M["grid"])
    out["obstacle grid"] = sum(count(M["grid"][k]["data"], np.asarray(R["occ"][k], np.int8)) for k in range(n))
    out["scan"] = sum(count(M["scan"][k]["ranges"], np.asarray(R["ranges"][k], np.float32)) for k in range(n))
    out["costmap"] = sum(count(M["costmap"][k]["data"], np.asarray(R["grid"][k], np.int8)) for k in range(n))
    out["inflated grid"] = count(M["inflated"][-1]["data"], nm.grid_value_of_cost(R["cost"]))
    src = M["costmap"][-1]
    xy = np.asarray(M["plan"][-1]["positions"])[:, :2]
    cells = np.rint((xy - src["origin"][:2]) / src["resolution"] - 0.5).astype(np.int32)
    out["path cells"] = count(cells, np.asarray(R["path"][:int(R["nav_stats"][2])], np.int32))
    lv, lw = nm.lattice(rp)
    best = int(np.abs(lv - M["cmd"][-1]["linear"][0]).argmin()) * rp.nw + int(np.abs(lw - M["cmd"][-1]["angular"][2]).argmin())
    out["best sample"] = count(np.uint32(best), np.uint32(R["best"][1]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(st.SCENES))
def test_node_messages_against_the_truth(harness, eng, name):
    M = harness.scene(name)
    checks = nt.CHECKS
    bad = nt.failures(name, M, nm.Decoder(), checks)
    R = ct.run_chain(st.SCENES[name], Engine(eng))
    diff = differing_bytes(M, R, ct.RP)
    print(f"{nt.TAG} {name} | bytes | differing from the api chain on the same maps: " + ", ".join(f"{k} {v}" for k, v in diff.items()))
    assert not bad, (bad, diff)
    # the level scenes are handed the file's mount on both sides; the pitched ones fit theirs from the same map with the same
    # parameters, frame by frame in the node and as one batch in the chain, which sn_ground_from_raw's contract makes the same
    assert not any(diff.values()), diff


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["free end", "gap and box", "corridor", "free end pitched"])
def test_the_mirrored_world_in_the_node(harness, name):
    nt.check_mirror(name, name + " mirrored", harness.scene(name), harness.scene(name + " mirrored"), nm.Decoder())


@pytest.mark.gpu
def test_the_far_pose(harness):
    """3 km from the origin, on a cell's border: the plan's first pose and the window's origin name the cell the truth names"""
    scene = st.FREE_END
    raws = st.render(scene, scene.poses[0])[None]
    goal = ((nt.FAR_CELL[0] + 10.5) * ct.CELL, (nt.FAR_CELL[1] + 0.5) * ct.CELL)      # a metre ahead, short of the wall the map shows
    M = harness.run("far pose", scene, [nt.FAR_POSE], goal, raws, (100, 100))
    nt.check_far_pose(M, nm.Decoder(), (100, 100))
    xy = np.asarray(M["plan"][-1]["positions"])[:, :2]
    assert float(np.hypot(*(xy[-1] - goal))) <= ct.SQ2 / 2 * ct.CELL + 1e-9, "the plan does not end in the goal's cell"
