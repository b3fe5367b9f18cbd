"""The `key value...` files of the node's stages, read by both readers: the node's (csrc/compat/src/param_file.cpp under the
tables of stage_files.cpp, run as the stand-alone program param_file_check under AddressSanitizer and
UndefinedBehaviorSanitizer) and the tools' (hobot_stereonet_amd/paramfile.py under each module's load_params).  No GPU and no
library.

The node's defaults are held to the Python dataclasses' field by field, and over every single-line mutation of a saved file
the two readers agree on accept or reject and, where they accept, on every value.  Left out on purpose, and written down in
DESIGN.md: numbers that only one of strtod and Python's int() / float() takes (`1e3` or `0x10` for an integer, `1_0`), and
integers outside the node's int32 / uint32 range."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import costmap, elevation, ground, inflate, navfn, obstacles, rectify, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
PROGRAM = os.path.join(COMPAT, "build", "param_file_check")

MOUNT = tuple(float(np.float32(v)) for v in np.linspace(-1.3, 2.7, 12))
_K = np.array([[500.5, 0, 320.25], [0, 499.75, 239.5], [0, 0, 1]])
CALIB = rectify.stereo_rectify(_K, [0.1, -0.05, 0.001, 0.002, 0.01], _K + np.diag([0.5, 0.5, 0.0]), [0.09, -0.04, 0.0, 0.001, 0.0],
                               rectify.rodrigues([0.01, -0.02, 0.005]), [-120.0, 1.0, 0.5], (640, 480), (64, 48))

# kind -> (module, a parameter set with no field at its default, the fields that only the tools read)
KINDS = {
    "obstacle": (obstacles, obstacles.ObstacleParams(
        base_from_cam=MOUNT, x_min_m=1.0, y_min_m=-2.125, cell_m=0.05, gw=37, gh=41, z_floor_m=-0.3, z_lo_m=0.07, z_hi_m=1e-7,
        min_obstacle_hits=2, min_ground_hits=5, beams=90, angle_min_rad=-0.7, angle_increment_rad=1.4 / 90, range_min_m=0.2, range_max_m=1e22,
        frame="cam_base"), ()),
    "ground": (ground, ground.GroundParams(
        base_from_cam=obstacles.mount(0.1, 0.2, (0.0, 0.1, 1.2)), roi_x=3, roi_y=5, roi_w=100, roi_h=64, hypotheses=77, seed=4294967295, min_area=9,
        min_inliers=11, refits=4, tol_px=0.25, max_tilt_rad=1.0, height_min_m=0.3, height_max_m=2.2, log_delta=0.5), ()),
    "costmap": (costmap, costmap.CostmapParams(
        mw=33, mh=65, l_hit=70, l_miss=30, l_min=-100, l_max=120, clear_margin_m=0.15, clear_min_m=0.3, clear_max_m=4.0, frame="map"), ()),
    "elevation": (elevation, elevation.ElevationParams(
        mw=64, mh=48, cell_m=0.05, base_from_cam=MOUNT, z_min_m=-0.5, z_max_m=1.25, range_max_m=4.5, min_points=2, alpha=200, max_step_mm=45,
        radius=2, flags=4, frame="map", feed_inflate=1), ()),
    "inflate": (inflate, inflate.InflateParams(cell_m=0.1, inscribed_radius_m=0.31, inflation_radius_m=0.77, cost_scaling=3.0, lethal_min=65, flags=1), ()),
    "plan": (navfn, navfn.NavParams(neutral=40, lethal_cost=200, unknown_cost=7, flags=1, max_rounds=123, max_path=999, goal=(5, 6), start=(1, 2)),
             ("goal", "start")),
    "rollout": (rollout, rollout.RolloutParams(
        cell_m=0.1, v_min=-0.1, v_max=0.9, nv=5, w_min=-0.5, w_max=0.75, nw=7, sim_time_s=2.0, steps=9, lethal_cost=250, centre_lethal_cost=240,
        unknown_cost=3, flags=1, w_goal=3, w_occ=2, footprint=((0.2, 0.1), (0.2, -0.1), (-0.2, -0.1), (-0.2, 0.1)), pose=(1.5, 2.0, 0.3),
        acc=(0.5, 1.0, 0.1)), ("pose",)),
}


@pytest.fixture(scope="module")
def program():
    subprocess.check_call(["make", "-C", COMPAT, "-s", "build/param_file_check"])
    return PROGRAM


def test_param_file_check_runs_clean_under_the_sanitizers(program):
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "param_file_check: ok" in run.stdout


def f32(v) -> str:
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]


def f64(v) -> str:
    return "0x%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def dumps(program, kind, paths):
    """-> per path, the error line or {key: [words] (for `point`, a list of them)} of param_file_check dump"""
    run = subprocess.run([program, "dump", kind] + list(paths) + ["/dev/null"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for block in run.stdout.split("== ")[1:]:
        path, _, body = block.partition("\n")
        if body.startswith("error "):
            out[path] = body.strip()
            continue
        got = out[path] = {}
        for line in body.splitlines():
            key, *words = line.split()
            if key == "point":
                got.setdefault(key, []).append(words)
            else:
                assert key not in got, line
                got[key] = words
    return [out[p] for p in paths]


def expected(kind, p):
    """what the dump must hold for the loaded parameters p: every field of the struct and every side output of the node"""
    if kind == "calib":
        want = {"src_w": [str(p.src_w)], "src_h": [str(p.src_h)]}
        for name, e in (("left", p.left), ("right", p.right)):
            want.update({name + ".K": [f64(v) for v in (e.fx, e.fy, e.cx, e.cy)], name + ".D": [f64(v) for v in e.d], name + ".R": [f64(v) for v in e.R]})
        want.update({k: [f64(getattr(p, k))] for k in ("pfx", "pfy", "pcx", "pcy", "baseline_mm")})
        return want
    module, _, tools_only = KINDS[kind]
    want = {}
    for field in dataclasses.fields(p):
        k, v = field.name, getattr(p, field.name)
        if k in tools_only:
            continue
        if k == "footprint":
            if v:
                want["point"] = [[f32(x), f32(y)] for x, y in v]
        elif k == "acc":
            if v is not None:
                want[k] = [f64(x) for x in v]
        elif k == "base_from_cam":
            want[k] = [f32(x) for x in v]
        elif k == "frame":
            want[k] = [v]
        else:
            floats = getattr(module, "_FLOATS", ())
            assert (k in module._INTS or k == "feed_inflate") != (k in floats), k
            want[k] = [f32(v)] if k in floats else [str(int(v))]
    return want


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_nodes_defaults_are_the_dataclasss(program, kind, tmp_path):
    module, params, _ = KINDS[kind]
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    assert dumps(program, kind, [str(empty)])[0] == expected(kind, type(params)())


def mutations(lines, int_keys):
    """every single-line mutation of the file: the line dropped, doubled, its key misspelt, its values replaced by `x`, by two
    values and, for an integer key, by 1.5"""
    for i, line in enumerate(lines):
        if line.startswith("#"):
            continue
        key = line.split()[0]
        yield lines[:i] + lines[i + 1:]
        yield lines[:i] + [line, line] + lines[i + 1:]
        for new in [key + "x" + line[len(key):], key + " x", key + " 1 2"] + ([key + " 1.5" * (len(line.split()) - 1)] * (key in int_keys)):
            yield lines[:i] + [new] + lines[i + 1:]


@pytest.mark.parametrize("kind", ["calib"] + list(KINDS))
def test_both_readers_agree_on_every_mutation_of_a_saved_file(program, kind, tmp_path):
    if kind == "calib":
        load, params, int_keys = rectify.load_calib, CALIB, ("size",)
        rectify.save_calib(str(tmp_path / "saved.txt"), params)
    else:
        module, params, _ = KINDS[kind]
        load, int_keys = module.load_params, module._INTS + ("goal", "start", "feed_inflate")
        module.save_params(str(tmp_path / "saved.txt"), params)
        assert all(getattr(params, f.name) != f.default for f in dataclasses.fields(params)), "a field at its default tells nothing"
    saved = (tmp_path / "saved.txt").read_text().splitlines()
    files = [saved] + list(mutations(saved, int_keys))
    paths = []
    for n, lines in enumerate(files):
        paths.append(str(tmp_path / f"m{n}.txt"))
        with open(paths[-1], "w") as f:
            f.write("".join(line + "\n" for line in lines))
    assert load(paths[0]) == params
    accepted = 0
    for path, lines, got in zip(paths, files, dumps(program, kind, paths)):
        try:
            want = expected(kind, load(path))
        except ValueError as e:
            assert isinstance(got, str), f"the node takes what {load.__module__} refuses ({e}):\n" + "\n".join(lines)
            assert path in str(e)
            continue
        assert got == want, "\n".join(lines)
        accepted += 1
    assert 1 < accepted < len(files)      # the saved file, a line dropped or a frame renamed; and most mutations are refused
