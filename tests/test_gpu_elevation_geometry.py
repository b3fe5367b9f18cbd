"""sn_elevation_push on the MI355X on every geometry, slice and limit it accepts (the inputs are tests/golden/elevation_domain.py,
judged on the CPU by tests/test_elevation_geometry.py): the geometries of postproc_domain.GEOMETRIES, and 300 x 20 for two column
blocks of two row chunks, at camera step 1, 2 and 4 in device mode on a caller's stream and in host mode, with mounts from device
memory and with outputs one element off 16-byte alignment; a push of 130 maps on three streams with a mount per map (launches of
64, 64 and 2 maps), then 70 more after a reset; 64 maps of 3 x 520 (the launcher's workgroup cap lengthens the row chunks); a
window of more cells than one pass of k_el_clear; windows of 4096 cells; poses on the quantiser's limit; and the node's fitted
mount of every frame reaching the elevation map.  Everywhere trav, hi, lo, rise and stats equal the twin's bytes (the twin fed the
library's q), with 16 guard bytes of 0x5a around every output.  No tolerance appears."""
import dataclasses

import numpy as np
import pytest

import elevation_domain as ed
from hobot_stereonet_amd import api, ground, inflate, obstacles, synth, weights
from hobot_stereonet_amd import elevation as el

GUARD = 16
NAMES = ("trav", "hi", "lo", "rise", "stats")
DTYPES = (np.int8, np.int16, np.int16, np.uint16, np.uint32)
ALL = (True,) * 5
GEOMS = list(ed.SWEEP)      # postproc_domain.GEOMETRIES and one geometry with two column blocks of two row chunks


def _sizes(n, p):
    c = n * p.mw * p.mh
    return (c, 2 * c, 2 * c, 2 * c, n * 16)


def _device(torch, ev, p, poses, raw, cam, mounts=None, stride=12, ids=None, want=ALL, stream=0, off=False):
    """device mode, as tests/test_gpu_elevation.py's: the maps (and mounts, `stride` floats apart) uploaded, every wanted output
    GUARD bytes into a buffer of 0x5a of its own (off: one element more, so no output is 16-byte aligned and each keeps the
    alignment of its type) -> (the five outputs (None where not wanted), q), after checking every byte the call must not write"""
    n = len(poses)
    d_raw = torch.from_numpy(np.array(raw, np.int32)).cuda()      # a copy: the domain's arrays are read-only
    d_m = None
    if mounts is not None:
        wide = np.full((n, stride), 7.0, np.float32)
        wide[:, :12] = np.asarray(mounts, np.float32).reshape(n, 12)
        d_m = torch.from_numpy(wide).cuda()
    lead = [GUARD + (np.dtype(d).itemsize if off else 0) for d in DTYPES]
    bufs = [torch.full((s + 2 * GUARD + 16,), 0x5a, dtype=torch.uint8, device="cuda") if w_ else None for s, w_ in zip(_sizes(n, p), want)]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() + a if b is not None else 0 for b, a in zip(bufs, lead)]
    assert all(b is None or b.data_ptr() % 16 == 0 for b in bufs)
    q = ev.push_device(n, poses, d_raw.data_ptr(), cam, d_m.data_ptr() if d_m is not None else 0, stride, ids, *ptrs, stream=stream)
    torch.cuda.synchronize()
    parts = []
    for name, b, s, a, d in zip(NAMES, bufs, _sizes(n, p), lead, DTYPES):
        if b is None:
            parts.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[:a] == 0x5a) and np.all(o[a + s:] == 0x5a), f"guard bytes around {name}"
        parts.append(o[a:a + s].copy().view(d).reshape((n, 4) if name == "stats" else (n, p.mh, p.mw)))
    assert np.array_equal(d_raw.cpu().numpy(), raw), "the maps were written to"
    return parts, q


def _differing(got, want, rows=slice(None)):
    """-> {name: number of differing elements} over the outputs that were asked for (a mis-shaped one counts whole)"""
    bad = {}
    for name, g, t in zip(NAMES, got, want):
        if g is None:
            continue
        g, t = g[rows], t[rows]
        if g.dtype != t.dtype or g.shape != t.shape:
            bad[name] = t.size
        elif g.tobytes() != np.ascontiguousarray(t).tobytes():
            bad[name] = int((g != t).sum())
    return bad


# ---- the geometry sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GEOMS, ids=[f"{w}x{h}" for w, h in GEOMS])
def test_the_elevation_map_equals_its_twin_at_this_geometry(model_factory, w, h):
    import torch
    bad = {}
    with api.StereoNetHIP(model_factory(w, h, ed.DMAX), max_batch=ed.N) as eng:
        stream = torch.cuda.Stream()
        for step in ed.STEPS:
            p, cam, poses, raw = ed.case(w, h, step)
            runs = {}
            with eng.elevation(p) as ev:
                with torch.cuda.stream(stream):
                    got, q = _device(torch, ev, p, poses, raw, cam, stream=stream.cuda_stream)
                assert np.array_equal(q, api.elevation_pose_q(p, poses))
                want = el.Reference(p).push(q, raw, cam)
                runs["device"] = _differing(got, want)
                ev.reset()
                host = ev.push(poses, raw, cam)
                assert np.array_equal(host[5], q)
                runs["host"] = _differing(host[:5], want)
                if step == 1:
                    ev.reset()                         # a mount per map from device memory, 16 floats apart: k_el_scatter<true>
                    mounts = np.asarray([obstacles.mount(0.0, 0.002 * k, (0.0, 0.0, 0.01 * k)) for k in range(ed.N)], np.float32)
                    with torch.cuda.stream(stream):
                        got, q2 = _device(torch, ev, p, poses, raw, cam, mounts=mounts, stride=16, stream=stream.cuda_stream)
                    mounted = el.Reference(p).push(q2, raw, cam, mounts)
                    assert w * h < 3 or mounted[4][0, 3] > 0, "no point was used under the mounts"
                    runs["mounts"] = _differing(got, mounted)
                    ev.reset()                         # no output 16-byte aligned
                    with torch.cuda.stream(stream):
                        got, _ = _device(torch, ev, p, poses, raw, cam, stream=stream.cuda_stream, off=True)
                    runs["off"] = _differing(got, want)
            print(f"elevation_geometry {w}x{h} step {step}: stats {want[4].tolist()}; differing elements "
                  + ", ".join(f"{k} {sum(v.values())}" for k, v in runs.items()))
            bad.update({(step, k): v for k, v in runs.items() if v})
    assert not bad, bad


# ---- the slice walk --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk_engine(model_factory):
    with api.StereoNetHIP(model_factory(ed.WALK_W, ed.WALK_H, ed.DMAX), max_batch=ed.BIG) as e:
        yield e


def _walk(torch, eng, mode, want=ALL):
    """the flow of the slice walk in one mode -> [(tag, outputs, the fresh twin's outputs, the twin's frames)] of the two pushes"""
    poses, raw, mounts = ed.walk()
    twin = el.Reference(ed.WALK, 3)
    done = []
    with eng.elevation(ed.WALK, streams=3) as ev:
        def push(ps, maps, ms, ids):
            if mode == "device":
                got, q = _device(torch, ev, ed.WALK, ps, maps, ed.WALK_CAM, mounts=ms, stride=16, ids=ids, want=want)
            else:
                r = ev.push(ps, maps, ed.WALK_CAM, ms, ids, want=want)
                got, q = list(r[:5]), r[5]
            assert np.array_equal(q, api.elevation_pose_q(ed.WALK, ps))
            first = len(twin.frames)
            done.append((f"{len(ps)} maps", got, twin.push(q, maps, ed.WALK_CAM, ms, ids), twin.frames[first:]))

        def reset(s):
            ev.reset(s)
            twin.reset(s)

        ed.walk_flow(push, reset)
    done[1] = ("70 maps after reset(1)",) + done[1][1:]
    return done


def _judge_walk(mode, done):
    bad = []
    for tag, got, want, _ in done:
        n = len(want[4])
        per = [sum(_differing(got, want, slice(k0, k0 + m)).values()) for k0, m in zip(range(0, n, ed.SLICE), ed.launches(n))]
        total = _differing(got, want)
        print(f"elevation_geometry slice walk, {mode}, {tag}: launches of {ed.launches(n)} maps, differing elements per launch {per}, "
              f"in all {total or 0}")
        if total:
            bad.append((mode, tag, per, total))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device", "host"])
def test_elevation_push_walks_three_slices(walk_engine, mode):
    import torch
    done = _walk(torch, walk_engine, mode)
    # the window moved inside every launch, and on the first map of launches two and three whose stream has a past
    ids1, _ = ed.walk_ids()
    frames = done[0][3]
    moved = [f["prev"] not in (None, f["origin"]) for f in frames]
    per_launch = [sum(moved[k0:k0 + m]) for k0, m in zip(range(0, ed.BIG, ed.SLICE), ed.launches(ed.BIG))]
    taken = {k: sum(f[k] for f in frames) for k in ("scrolled", "born", "blended", "up", "down")}
    print(f"elevation_geometry slice walk, {mode}: the window moved {per_launch} times in the three launches; branches taken {taken}")
    assert ed.launches(ed.BIG) == [64, 64, 2] and ed.launches(ed.SECOND) == [64, 6]
    assert all(per_launch) and all(taken.values())
    for k0 in (ed.SLICE, 2 * ed.SLICE):
        k = next(k for k in range(k0, ed.BIG) if ids1[k] in ids1[:k0])
        assert moved[k], k
    bad = _judge_walk(mode, done)
    assert not bad, bad


@pytest.mark.gpu
def test_elevation_push_walks_three_slices_with_stats_alone(walk_engine):
    """only stats wanted: hi and lo are the scratch planes, cut per slice like the caller's"""
    import torch
    bad = _judge_walk("device, stats alone", _walk(torch, walk_engine, "device", want=(False, False, False, False, True)))
    assert not bad, bad


@pytest.mark.gpu
def test_a_launch_whose_row_chunks_the_workgroup_cap_shortens(model_factory):
    """64 maps of 3 x 520: the launcher's cap of about 2048 workgroups gives 31 chunks of 17 rows where every other test runs
    chunks of 16"""
    import torch
    assert ed.cap_chunks() == (31, 17)
    poses, raw = ed.capped()
    with api.StereoNetHIP(model_factory(ed.CAP_W, ed.CAP_H, ed.DMAX), max_batch=ed.CAP_N) as e, e.elevation(ed.BASE) as ev:
        got, q = _device(torch, ev, ed.BASE, poses, raw, ed.CAP_CAM)
        want = el.Reference(ed.BASE).push(q, raw, ed.CAP_CAM)
        diff = _differing(got, want)
        ev.reset()
        host = ev.push(poses, raw, ed.CAP_CAM)
        diff_host = _differing(host[:5], want)
    print(f"elevation_geometry capped launch, {ed.CAP_N} maps of {ed.CAP_W}x{ed.CAP_H}: points per map {int(want[4][:, 3].min())} to "
          f"{int(want[4][:, 3].max())}; differing elements device {sum(diff.values())}, host {sum(diff_host.values())}")
    assert want[4][:, 3].min() > 0
    assert not diff and not diff_host, (diff, diff_host)


# ---- windows: more cells than one pass of the clear, and the declared limit ----------------------------------------------------------
@pytest.fixture(scope="module")
def eng(model_factory):
    with api.StereoNetHIP(model_factory(ed.BIG_W, ed.BIG_H, ed.DMAX), max_batch=4) as e:
        yield e


@pytest.mark.gpu
def test_more_cells_than_one_pass_of_the_clear(eng):
    """3 x 700 x 260 cells: the grid-stride loop of k_el_clear takes a second pass.  The clip is pushed twice in each mode, so the
    second push finds the first's accumulators in the scratch: cells the clear left out would count their points twice."""
    import torch
    p = ed.BIG_WINDOW
    poses, raw = ed.big_window()
    assert ed.N * p.mw * p.mh > ed.CLEAR_PASS
    with eng.elevation(p) as ev:
        twin = el.Reference(p)
        wants = []
        for mode in ("device", "host"):
            ev.reset()
            twin.reset()
            for turn in range(2):
                if mode == "device":
                    got, q = _device(torch, ev, p, poses, raw, ed.CAM)
                else:
                    r = ev.push(poses, raw, ed.CAM)
                    got, q = list(r[:5]), r[5]
                if len(wants) <= turn:
                    wants.append(twin.push(q, raw, ed.CAM))
                diff = _differing(got, wants[turn])
                print(f"elevation_geometry big window {p.mw}x{p.mh} x {ed.N}, {mode}, push {turn}: stats {wants[turn][4].tolist()}; "
                      f"differing elements {sum(diff.values())}")
                assert not diff, (mode, turn, diff)
    assert wants[0][4][:, 0].min() >= 1000


@pytest.mark.gpu
@pytest.mark.parametrize("mw,mh", ed.LIMITS)
def test_windows_at_the_declared_limit(eng, mw, mh):
    import torch
    p, poses, raw = ed.limit_case(mw, mh)
    with eng.elevation(p) as ev:
        got, q = _device(torch, ev, p, poses, raw, ed.LIMIT_CAM)
        want = el.Reference(p).push(q, raw, ed.LIMIT_CAM)
        diff = _differing(got, want)
        ev.reset()
        host = ev.push(poses, raw, ed.LIMIT_CAM)
        diff_host = _differing(host[:5], want)
    print(f"elevation_geometry window {mw}x{mh}: stats {want[4].tolist()}; differing elements device {sum(diff.values())}, host {sum(diff_host.values())}")
    assert want[4][:, 2].min() >= 10, "the window receives too few points"
    assert not diff and not diff_host, (diff, diff_host)


@pytest.mark.gpu
def test_poses_at_the_far_limit(eng):
    """|x| * k256 = |y| * k256 = 2^30 in both signs, yaw near pi and -pi, then a step back across the last cell boundary"""
    import torch
    p = ed.FAR
    poses, raw, ids = ed.far_poses()
    with eng.elevation(p, streams=2) as ev:
        got, q = _device(torch, ev, p, poses, raw, ed.CAM, ids=ids)
        assert np.array_equal(q, api.elevation_pose_q(p, poses)) and np.array_equal(ev.pose_q(poses), q)
        assert q[0, 0] == 1 << 30 and q[0, 1] == -(1 << 30) and q[2, 0] == -(1 << 30) and q[2, 1] == 1 << 30
        twin = el.Reference(p, 2)
        want = twin.push(q, raw, ed.CAM, stream_of=ids)
        diff = _differing(got, want)
        ev.reset()
        host = ev.push(poses, raw, ed.CAM, stream_of=ids)
        diff_host = _differing(host[:5], want)
    print(f"elevation_geometry far poses: q {q[:, :2].tolist()}, origins {q[:, 4:].tolist()}, stats {want[4].tolist()}; "
          f"differing elements device {sum(diff.values())}, host {sum(diff_host.values())}")
    assert want[4][:, 0].min() >= 10 and all(f["prev"] != f["origin"] for f in (twin.frames[1], twin.frames[3]))
    assert not diff and not diff_host, (diff, diff_host)


# ---- the node: the frame's fitted mount reaches the elevation map ------------------------------------------------------------------
def _fit_under(raw, cam, mount):
    """parameters under which the map fills a good part of a 21 x 18 window when it is seen under `mount`: cells a fifth of the
    median range, every height the stage accepts (test_gpu_elevation_tools._fit, under a mount)"""
    xb, yb, zb = el.base_points(raw[None], cam, np.asarray(mount, np.float32)[None])
    r = np.hypot(xb, yb)[np.isfinite(zb)]
    assert r.size > 100
    cell = float(np.float32(np.median(r) / 5.0))
    return el.ElevationParams(mw=21, mh=18, cell_m=cell, z_min_m=-30.0, z_max_m=30.0, range_max_m=float(np.float32(20 * cell)), min_points=2,
                              alpha=128, max_step_mm=max(1, min(32767, int(1000 * cell))), radius=2, frame="map")


@pytest.mark.gpu
def test_node_gives_the_elevation_map_every_frames_mount(weights_blob, tmp_path):
    """STEREONET_GROUND beside STEREONET_ELEVATION: /stereonet_traversability carries the twin chain's bytes (the plane of the
    frame's map, its mount, the elevation map pushed with that mount), not those of the elevation file's own mount; the inflated
    grid follows exactly those bytes; a ground file the stage refuses leaves the elevation map with its file's mount"""
    import subprocess
    from hobot_stereonet_amd import build
    from test_gpu_elevation_tools import CAM, CAM_ENV, COMPAT, D, H, W, _run_harness
    from test_gpu_ground import _found_params
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    nframes = 3
    m, f_bin = str(tmp_path / "m.snw"), str(tmp_path / "f.bin")
    weights.save_snw(m, weights_blob, W, H, D)
    sbs = synth.sbs_nv12_frame(W, H, D, 70)
    np.asarray(sbs).tofile(f_bin)
    with api.StereoNetHIP(m) as e:
        first = e.infer_sbs_nv12(sbs)[1].reshape(H, W)
    gp = _found_params(first, CAM, base_from_cam=obstacles.mount(0.0, 0.0, (0.0, 0.0, 0.3)), log_delta=0.001)
    gate = api.ground_gate(CAM, gp, W, H)
    rec0, _ = ground.reference(first, CAM, gp, gate_q16=gate, labels=False)
    p = _fit_under(first, CAM, rec0["base_from_cam"])
    ip = inflate.InflateParams(cell_m=0.05, inscribed_radius_m=1.2 * p.cell_m, inflation_radius_m=2.5 * p.cell_m, cost_scaling=1.0, lethal_min=100, flags=0)
    el.save_params(str(tmp_path / "el.txt"), p)
    el.save_params(str(tmp_path / "el_feed.txt"), dataclasses.replace(p, feed_inflate=1))
    ground.save_params(str(tmp_path / "ground.txt"), gp)
    ground.save_params(str(tmp_path / "bad.txt"), dataclasses.replace(gp, hypotheses=0))
    inflate.save_params(str(tmp_path / "in.txt"), ip)
    poses = np.array([[0.0, 0.0, 0.0], [2 * p.cell_m, 0.5 * p.cell_m, 0.2], [-1 * p.cell_m, -3 * p.cell_m, -0.4]])
    env = dict(CAM_ENV, STEREONET_ELEVATION=str(tmp_path / "el.txt"))
    plain, _, _, _, _ = _run_harness(tmp_path, "file", m, f_bin, nframes, env, poses)
    msgs, travs, infl, order, log = _run_harness(tmp_path, "fit", m, f_bin, nframes, dict(env, STEREONET_GROUND=str(tmp_path / "ground.txt")), poses)
    assert msgs == plain and len(travs) == nframes and not infl and order == ["traversability"] * nframes and "ground: found, height" in log
    q = api.elevation_pose_q(p, poses)
    twin, own = el.Reference(p), el.Reference(p)
    differs = 0
    for k in range(nframes):
        raw = np.frombuffer(msgs[k][:4 * W * H], np.int32).reshape(H, W)
        rec, _ = ground.reference(raw, CAM, gp, gate_q16=gate, labels=False)
        assert rec["flags"] & ground.FOUND
        want = twin.push(q[k:k + 1], raw[None], CAM, np.asarray(rec["base_from_cam"], np.float32).reshape(1, 12))
        file_mount = own.push(q[k:k + 1], raw[None], CAM)
        fit_bytes, file_bytes = open(tmp_path / f"fit.{k}.trav", "rb").read(), open(tmp_path / f"file.{k}.trav", "rb").read()
        print(f"elevation_geometry node, frame {k}: stats under the fitted mount {want[4][0].tolist()}, under the file's {file_mount[4][0].tolist()}; "
              f"differing bytes {sum(a != b for a, b in zip(fit_bytes, want[0].tobytes()))} and "
              f"{sum(a != b for a, b in zip(file_bytes, file_mount[0].tobytes()))}; the two grids differ in "
              f"{sum(a != b for a, b in zip(fit_bytes, file_bytes))} cells")
        assert fit_bytes == want[0].tobytes() and file_bytes == file_mount[0].tobytes(), k
        assert [int(travs[k]["known"]), int(travs[k]["lethal"])] == want[4][0, :2].tolist()
        assert (want[0] >= 0).sum() >= 10, "the window is nearly empty: the check says little"
        differs += fit_bytes != file_bytes
    assert differs == nframes
    # feed_inflate 1: the inflated grid is the twin's of exactly the bytes under the fitted mount
    table = api.inflate_table(dataclasses.replace(ip, cell_m=p.cell_m))
    feed_env = dict(CAM_ENV, STEREONET_ELEVATION=str(tmp_path / "el_feed.txt"), STEREONET_GROUND=str(tmp_path / "ground.txt"),
                    STEREONET_INFLATE=str(tmp_path / "in.txt"))
    msgs, travs, infl, order, log = _run_harness(tmp_path, "feed", m, f_bin, nframes, feed_env, poses)
    assert msgs == plain and order == ["traversability", "inflated"] * nframes and "feeding the inflation" in log
    for k in range(nframes):
        trav = np.fromfile(str(tmp_path / f"feed.{k}.trav"), np.int8).reshape(1, p.mh, p.mw)
        assert trav.tobytes() == open(tmp_path / f"fit.{k}.trav", "rb").read(), k
        want = inflate.reference(trav, dataclasses.replace(ip, cell_m=p.cell_m), table)[1]
        assert open(tmp_path / f"feed.{k}.inflated", "rb").read() == want.tobytes(), k
    # a ground file the stage refuses: the elevation map keeps its file's mount
    msgs, travs, infl, order, log = _run_harness(tmp_path, "bad", m, f_bin, nframes, dict(env, STEREONET_GROUND=str(tmp_path / "bad.txt")), poses)
    assert msgs == plain and len(travs) == nframes and log.count("no ground plane") == 1
    for k in range(nframes):
        assert open(tmp_path / f"bad.{k}.trav", "rb").read() == open(tmp_path / f"file.{k}.trav", "rb").read(), k
