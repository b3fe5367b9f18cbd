"""sn_elevation behind the node and the filelist tool on the MI355X: /stereonet_traversability carries the twin's bytes at the
poses of SetBasePose with the header of the frame; `feed_inflate 1` makes it the source of /stereonet_inflated_grid, with and
without the obstacle stage; without STEREONET_ELEVATION, or without that line, every message the node published before is the
same bytes; `filelist --elevation` writes the twin's pictures and counts."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import api, inflate, obstacles, synth, weights
from hobot_stereonet_amd import elevation as el
from hobot_stereonet_amd.elevation import ElevationParams
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H, D = 96, 64, 48
CAM = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0, z_min_m=0.05)
CAM_ENV = {"STEREONET_CAMERA": "80,80,47.5,20.5,120", "STEREONET_POINTCLOUD_Z": "0.05,0"}


def _fit(raw, cam) -> ElevationParams:
    """parameters under which the map of a model with synthetic weights fills a good part of a 21 x 18 window: cells a fifth of
    the median range, every height"""
    xb, yb, zb = el.base_points(raw[None], cam, np.asarray(obstacles.LEVEL_MOUNT, np.float32)[None])
    r = np.hypot(xb, yb)[np.isfinite(zb)]
    assert r.size > 100
    cell = float(np.float32(np.median(r) / 5.0))
    return ElevationParams(mw=21, mh=18, cell_m=cell, z_min_m=-30.0, z_max_m=30.0, range_max_m=float(np.float32(20 * cell)), min_points=2, alpha=128,
                           max_step_mm=max(1, min(32767, int(1000 * cell))), radius=2, frame="map")


def _run_harness(tmp_path, tag, model, frames, nframes, env_extra, poses=None):
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("STEREONET_")}, SN_LOG_LEVEL="2", **env_extra)
    prefix = str(tmp_path / tag)
    args = [os.path.join(COMPAT, "build", "elevation_harness"), model, frames, str(W), str(H), str(nframes), prefix]
    if poses is not None:
        path = str(tmp_path / f"{tag}.poses")
        with open(path, "w") as f:
            f.write("".join(f"{float(x)!r} {float(y)!r} {float(yaw)!r}\n" for x, y, yaw in poses))
        args.append(path)
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    msgs = [open(f"{prefix}.{i}.msg", "rb").read() for i in range(nframes)]
    travs = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("traversability ")]
    infl = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in lines if l.startswith("inflated ")]
    order = [l.split()[0] for l in lines if l.split()[0] in ("traversability", "inflated")]
    return msgs, travs, infl, order, r.stdout + r.stderr


@pytest.mark.gpu
def test_node_publishes_the_traversability_grid(weights_blob, tmp_path):
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 3
    m = str(tmp_path / "m.snw")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(str(tmp_path / "f.bin"))
    f_bin = str(tmp_path / "f.bin")
    with api.StereoNetHIP(m) as e:
        p = _fit(e.infer_sbs_nv12(sbs)[1].reshape(H, W), CAM)
    el.save_params(str(tmp_path / "el.txt"), p)
    el.save_params(str(tmp_path / "el_feed.txt"), dataclasses.replace(p, feed_inflate=1))
    ip = InflateParams(cell_m=0.05, inscribed_radius_m=1.2 * p.cell_m, inflation_radius_m=2.5 * p.cell_m, cost_scaling=1.0, lethal_min=100, flags=0)
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    op = ObstacleParams(x_min_m=0.0, y_min_m=-8 * p.cell_m, cell_m=p.cell_m, gw=12, gh=16, z_floor_m=-30.0, z_lo_m=0.0, z_hi_m=30.0, frame="base_footprint")
    obstacles.save_params(str(tmp_path / "ob.txt"), op)
    plain, t0, i0, order, _ = _run_harness(tmp_path, "plain", m, f_bin, nframes, CAM_ENV)
    assert not t0 and not i0 and not order                                       # unset: nothing on the topic
    poses = np.array([[0.0, 0.0, 0.0], [2 * p.cell_m, 0.5 * p.cell_m, 0.2], [-1 * p.cell_m, -3 * p.cell_m, -0.4]])
    for tag, ps in (("posed", poses), ("still", None)):                          # without SetBasePose: the origin for every frame
        msgs, travs, infl, order, log = _run_harness(tmp_path, tag, m, f_bin, nframes, dict(CAM_ENV, STEREONET_ELEVATION=str(tmp_path / "el.txt")), ps)
        assert msgs == plain and len(travs) == nframes and not infl and order == ["traversability"] * nframes and "/stereonet_traversability" in log
        q = api.elevation_pose_q(p, poses if ps is not None else np.zeros((nframes, 3)))
        raws = np.stack([np.frombuffer(msgs[k][:4 * W * H], np.int32).reshape(H, W) for k in range(nframes)])
        want = el.Reference(p).push(q, raws, CAM)
        assert (want[0] >= 0).sum() >= 10, "the window is nearly empty: the check says little"
        cell = float(np.float32(p.cell_m))
        for k in range(nframes):
            assert open(tmp_path / f"{tag}.{k}.trav", "rb").read() == want[0][k].tobytes(), (tag, k)
            g = travs[k]
            assert g["frame_id"] == "map" and g["stamp"] == f"7.{1000 + k}" and (int(g["width"]), int(g["height"]), int(g["len"])) == (21, 18, 21 * 18)
            assert np.float32(g["resolution"]) == np.float32(p.cell_m) and [int(g["known"]), int(g["lethal"])] == want[4][k, :2].tolist()
            assert [float(v) for v in g["origin"].split(",")] == [float(np.float64(f"{int(q[k, 4]) * cell:.9g}")), float(np.float64(f"{int(q[k, 5]) * cell:.9g}"))]
    # feed_inflate 1: the inflated grid follows the traversability grid, with its header and the twin's bytes, without an obstacle stage
    table = api.inflate_table(dataclasses.replace(ip, cell_m=p.cell_m))
    msgs, travs, infl, order, log = _run_harness(tmp_path, "feed", m, f_bin, nframes,
                                                 dict(CAM_ENV, STEREONET_ELEVATION=str(tmp_path / "el_feed.txt"), STEREONET_INFLATE=str(tmp_path / "in.txt")), poses)
    assert msgs == plain and order == ["traversability", "inflated"] * nframes and "feeding the inflation" in log
    for k in range(nframes):
        trav = np.fromfile(str(tmp_path / f"feed.{k}.trav"), np.int8).reshape(1, p.mh, p.mw)
        assert trav.tobytes() == open(tmp_path / f"posed.{k}.trav", "rb").read()
        want = inflate.reference(trav, dataclasses.replace(ip, cell_m=p.cell_m), table)[1]
        assert open(tmp_path / f"feed.{k}.inflated", "rb").read() == want.tobytes(), k
        assert {a: infl[k][a] for a in ("frame_id", "stamp", "width", "height", "resolution", "origin")} == \
               {a: travs[k][a] for a in ("frame_id", "stamp", "width", "height", "resolution", "origin")}
    # with the obstacle stage and the inflation on, and no feed_inflate line: the inflated grid is the obstacle grid's, byte for byte
    # what it is without STEREONET_ELEVATION
    both = dict(CAM_ENV, STEREONET_OBSTACLES=str(tmp_path / "ob.txt"), STEREONET_INFLATE=str(tmp_path / "in.txt"))
    _, _, infl_off, order_off, _ = _run_harness(tmp_path, "ob", m, f_bin, nframes, both, poses)
    _, travs, infl_on, order_on, _ = _run_harness(tmp_path, "obel", m, f_bin, nframes, dict(both, STEREONET_ELEVATION=str(tmp_path / "el.txt")), poses)
    assert order_off == ["inflated"] * nframes and order_on == ["inflated", "traversability"] * nframes
    for k in range(nframes):
        assert open(tmp_path / f"ob.{k}.inflated", "rb").read() == open(tmp_path / f"obel.{k}.inflated", "rb").read(), k
        assert {a: infl_on[k][a] for a in ("frame_id", "width", "height", "origin")} == {a: infl_off[k][a] for a in ("frame_id", "width", "height", "origin")}
        assert infl_on[k]["frame_id"] == "base_footprint" and open(tmp_path / f"obel.{k}.trav", "rb").read() == open(tmp_path / f"posed.{k}.trav", "rb").read()
    # ... and with the line the source changes
    _, travs, infl_fed, order_fed, _ = _run_harness(tmp_path, "obfeed", m, f_bin, nframes, dict(both, STEREONET_ELEVATION=str(tmp_path / "el_feed.txt")), poses)
    assert order_fed == ["traversability", "inflated"] * nframes and all(g["frame_id"] == "map" for g in infl_fed)
    for k in range(nframes):
        assert open(tmp_path / f"obfeed.{k}.inflated", "rb").read() == open(tmp_path / f"feed.{k}.inflated", "rb").read(), k
    # a file the stage refuses: the node is as it is without the variable
    el.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(p, radius=4))
    msgs, travs, infl, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, dict(CAM_ENV, STEREONET_ELEVATION=str(tmp_path / "bad.txt")))
    assert msgs == plain and not travs and not order and log.count("no elevation map") == 1


@pytest.mark.gpu
def test_filelist_writes_the_traversability_pictures(model_factory, tmp_path, capsys):
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
    cam = dataclasses.replace(CAM, z_min_m=0.0)
    model = model_factory(W, H, D)
    with api.StereoNetHIP(model) as e:
        eyes = [images.bgr_to_nv12(images.imread_bgr(str(tmp_path / f"{eye}0.ppm"))) for eye in ("left", "right")]
        p = _fit(e.infer_sbs_nv12(images.sbs_from_eyes(eyes[0], eyes[1], W, H))[1].reshape(H, W), cam)
    el.save_params(str(tmp_path / "el.txt"), p)
    poses = np.array([[0.0, 0.0, 0.0], [p.cell_m, 0.0, 0.2], [3 * p.cell_m, -p.cell_m, -0.3]])
    (tmp_path / "poses.txt").write_text("# x y yaw\n" + "".join(f"{float(x)!r} {float(y)!r} {float(yaw)!r}\n" for x, y, yaw in poses))
    common = ["--model", model, "--left", lists["left"], "--right", lists["right"], "--camera", "80,80,47.5,20.5,120"]
    with pytest.raises(SystemExit):
        filelist.main(common + ["--elevation", str(tmp_path / "el.txt")])      # needs --out
    capsys.readouterr()
    for tag, arg, ps in (("posed", f"{tmp_path / 'el.txt'},{tmp_path / 'poses.txt'}", poses), ("still", str(tmp_path / "el.txt"), np.zeros((n, 3)))):
        out = str(tmp_path / tag)
        assert filelist.main(common + ["--out", out, "--elevation", arg]) == 0
        summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        twin = el.Reference(p)
        q = api.elevation_pose_q(p, ps)
        for i in range(n):
            raw = np.fromfile(os.path.join(out, f"{i}.raw.bin"), np.int32).reshape(1, H, W)
            trav, hi, _, _, stats = twin.push(q[i:i + 1], raw, cam)
            head = f"P5\n{p.mh} {p.mw}\n255\n".encode()
            assert open(os.path.join(out, f"{i}.trav.pgm"), "rb").read() == head + el.trav_image(trav[0]).tobytes(), (tag, i)
            assert open(os.path.join(out, f"{i}.hi.pgm"), "rb").read() == head + el.height_image(hi[0]).tobytes(), (tag, i)
            assert [summary["elevation"][k][i] for k in ("known", "lethal", "fused")] == stats[0, :3].tolist() and stats[0, 0] > 0
        assert summary["frames"] == n
