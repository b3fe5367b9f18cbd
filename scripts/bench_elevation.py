#!/usr/bin/env python3
"""Times the rolling elevation map (device buffers, a caller stream, device events; after 5 warm-up calls the median of three
windows of at least 50 calls and a quarter of a second each, `spread` = (max - min) / median of the three) at the obstacle
bench's size: 1280x720 maps and a 400 x 400 window of 0.05 m cells.  sn_elevation_push at batch 64 as one clip (one stream, 64
frames: the state is read and written once), as 64 streams of one frame each, and at batch 1; each with all five outputs and
with the verdict alone.  In the same run, on the same box and the same maps: sn_obstacles_from_raw (occ and ranges) and
sn_infer_batch per pair, at batch 64 and 1.  Two kinds of maps: obstacles.ground_and_wall scenes (a level camera 0.5 m above
the ground, a wall that comes nearer from map to map) along a walk that scrolls the window, and the noise-like maps the forward
pass makes of synthetic frames under synthetic weights, the scatter's bad case (neighbouring pixels in unrelated cells).  The first
three frames of every configuration are compared with the numpy twin's bytes before anything is timed.  Prints one JSON line.

    python scripts/bench_elevation.py [--iters K] [--warmup W] [--out FILE]

The byte floor per map at the achievable HBM rate (6.3 TB/s, a float4 copy on this part): 4 bytes read per sample plus the
requested output planes (trav 1, hi 2, lo 2, rise 2 bytes a cell, 16 of statistics).  `fraction_of_floor` = floor time / measured.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd import elevation as el  # noqa: E402
from hobot_stereonet_amd.elevation import ElevationParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
HBM_BYTES_PER_S = 6.3e12
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
MOUNT = obstacles.mount(t=(0.0, 0.0, 0.5))
SCENE = ObstacleParams(base_from_cam=MOUNT, x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15, z_lo_m=0.1, z_hi_m=1.5,
                       beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
MAP = ElevationParams(mw=400, mh=400, cell_m=0.05, base_from_cam=MOUNT, z_min_m=-1.0, z_max_m=1.5, range_max_m=10.0, min_points=3, alpha=128,
                      max_step_mm=60, radius=2)
CASES = [("1 stream x 64 frames", N, None), ("64 streams x 1 frame", N, list(range(N))), ("n = 1", 1, None)]
OUTPUTS = {"all": (True, True, True, True, True), "trav": (True, False, False, False, False)}
PLANE_BYTES = (1, 2, 2, 2)


SPREAD = {}      # the last timed() call's (max - min) / median over its three windows


def timed(call, st, warmup, iters, window_s=0.25):
    """milliseconds per call: the median of three windows, each of at least `iters` calls and about window_s seconds"""
    def window(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(k):
            call()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / k
    for _ in range(warmup):
        call()
    st.synchronize()
    k = max(iters, min(5000, int(window_s * 1e3 / max(window(iters), 1e-3)) + 1))
    ms = sorted(window(k) for _ in range(3))
    SPREAD["last"] = (ms[2] - ms[0]) / ms[1]
    return ms[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    scene = np.stack([obstacles.ground_and_wall(W, H, CAM, 0.5, 6.0 - 0.05 * k) for k in range(N)])
    poses = np.stack([0.025 * np.arange(N), 0.4 * np.sin(np.arange(N) / 9.0), 0.3 * np.sin(np.arange(N) / 5.0)], axis=1)
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)])
    cells, ocells = MAP.mw * MAP.mh, SCENE.gw * SCENE.gh
    rows, stage = [], []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        st = torch.cuda.Stream()
        with api.StereoNetHIP(model, max_batch=N) as eng:
            d_sbs = torch.from_numpy(np.ascontiguousarray(np.tile(frames, (N // 4, 1)))).cuda()
            dx = torch.empty((N, 6, H, W), dtype=torch.int8, device="cuda")
            d_net = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
            eng.preprocess_sbs_nv12_device(N, d_sbs.data_ptr(), dx.data_ptr())
            torch.cuda.synchronize()
            fwd = {n: timed(lambda: eng.infer_device(n, dx.data_ptr(), d_net.data_ptr(), 0, st.cuda_stream), st, 3, 20) * 1e3 / n for n in (N, 1)}
            eng.infer_device(N, dx.data_ptr(), d_net.data_ptr(), 0, st.cuda_stream)      # every map of the noise scene
            torch.cuda.synchronize()
            del dx, d_sbs
            maps = {"ground and wall": torch.from_numpy(scene).cuda(), "forward noise": d_net}
            d_occ = torch.empty(N * ocells, dtype=torch.int8, device="cuda")
            d_rng = torch.empty(N * SCENE.beams, dtype=torch.float32, device="cuda")
            outs = (torch.empty(N * cells, dtype=torch.int8, device="cuda"), torch.empty(N * cells, dtype=torch.int16, device="cuda"),
                    torch.empty(N * cells, dtype=torch.int16, device="cuda"), torch.empty(N * cells, dtype=torch.int16, device="cuda"),
                    torch.empty(N * 4, dtype=torch.int32, device="cuda"))
            for kind, d_raw in maps.items():
                ob = {n: timed(lambda: eng.obstacles_device(n, d_raw.data_ptr(), CAM, SCENE, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr(),
                                                            stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3 / n for n in (1, N)}
                for n in (N, 1):
                    stage.append({"maps": kind, "n": n, "forward_us_per_pair": round(fwd[n], 3), "obstacles_us_per_map": round(ob[n], 3),
                                  "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
                raw3 = d_raw[:3].cpu().numpy()
                for name, n, ids in CASES:
                    streams = n if ids else 1
                    for what, sel in OUTPUTS.items():
                        ptrs = [t.data_ptr() if s else 0 for t, s in zip(outs, sel)]
                        with eng.elevation(MAP, streams=streams) as ev:
                            def call():
                                return ev.push_device(n, poses[:n], d_raw.data_ptr(), CAM, 0, 12, ids, *ptrs, stream=st.cuda_stream)
                            m = min(n, 3)      # the twin's bytes before the clock starts
                            q = ev.push_device(m, poses[:m], d_raw.data_ptr(), CAM, 0, 12, ids[:m] if ids else None, *ptrs)
                            want = el.Reference(MAP, streams).push(q, raw3[:m], CAM, stream_of=ids[:m] if ids else None)
                            for t, s, w_ in zip(outs, sel, want):
                                if s and t[:w_.size].cpu().numpy().tobytes() != w_.tobytes():
                                    raise SystemExit(f"{kind}, {name} ({what}): differs from the numpy twin")
                            ev.reset()
                            ms = timed(call, st, args.warmup, args.iters)
                        floor_bytes = 4 * W * H + sum(b * cells for b, s in zip(PLANE_BYTES, sel) if s) + (16 if sel[4] else 0)
                        us, floor_us = ms * 1e3 / n, floor_bytes / HBM_BYTES_PER_S * 1e6
                        rows.append({"maps": kind, "case": name, "outputs": what, "n": n, "streams": streams, "us": round(ms * 1e3, 3),
                                     "us_per_map": round(us, 3), "obstacles_us_per_map": round(ob[n], 3), "ratio_to_obstacles": round(us / ob[n], 4),
                                     "forward_us_per_pair": round(fwd[n], 3), "share_of_forward": round(us / fwd[n], 5),
                                     "floor_bytes_per_map": int(floor_bytes), "floor_us_per_map": round(floor_us, 4),
                                     "fraction_of_floor": round(floor_us / us, 5), "spread": round(SPREAD["last"], 4), "stats_of_map_0": [int(v) for v in want[4][0]]})
                        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = {"elevation_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "window": [MAP.mw, MAP.mh], "cell_m": MAP.cell_m, "radius": MAP.radius, "stages": stage,
           "elevation": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
