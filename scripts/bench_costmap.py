#!/usr/bin/env python3
"""Times the rolling costmap (device buffers, a caller stream, device events, 50 calls after 5 warm-up) at the obstacle bench's
size: 1280x720 maps, a 200 x 200 observation grid of 0.05 m cells, 360 beams, and a 400 x 400 window.  sn_costmap_push at batch
64 as one clip (one stream, 64 frames: the state is read and written once), as 64 streams of one frame each (the state of every
stream read and written), and at batch 1; each with all three outputs and with the grid alone.  In the same run, on the same
box and the same maps: sn_obstacles_from_raw (occ and ranges, what the costmap reads) and sn_infer_batch per pair, at batch 64
and 1.  The inputs are the obstacle stage's own outputs on obstacles.ground_and_wall scenes (a level camera 0.5 m above the
ground, a wall that comes nearer from map to map) along a walk that scrolls the window by a cell every other frame.  The first
three frames of every configuration are compared with the numpy twin's bytes before anything is timed.  Prints one JSON line.

    python scripts/bench_costmap.py [--iters K] [--warmup W] [--out FILE]

The byte floor per map at the achievable HBM rate (6.3 TB/s, a float4 copy on this part): per cell 2 bytes of state read and 2
written per stream and launch, the chosen outputs per frame (grid 1, logodds 2, 16 of statistics), plus the inputs read once
(1 byte a grid cell, 4 a beam).  `fraction_of_floor` = floor time / measured.
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

from hobot_stereonet_amd import api, costmap, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd.costmap import CostmapParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
HBM_BYTES_PER_S = 6.3e12
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
SCENE = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15,
                       z_lo_m=0.1, z_hi_m=1.5, beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
MAP = CostmapParams(mw=400, mh=400, l_hit=85, l_miss=40, l_min=-200, l_max=350, clear_margin_m=0.1, clear_min_m=0.2, clear_max_m=0.0)
CASES = [("1 stream x 64 frames", N, None), ("64 streams x 1 frame", N, list(range(N))), ("n = 1", 1, None)]
OUTPUTS = {"all": (True, True, True), "grid": (True, False, False)}


def timed(call, st, warmup, iters):
    for _ in range(warmup):
        call()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        call()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


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
            del dx, d_sbs, d_net
            d_raw = torch.from_numpy(scene).cuda()
            d_occ = torch.empty(N * ocells, dtype=torch.int8, device="cuda")
            d_rng = torch.empty(N * SCENE.beams, dtype=torch.float32, device="cuda")
            ob = {n: timed(lambda: eng.obstacles_device(n, d_raw.data_ptr(), CAM, SCENE, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr(),
                                                        stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3 / n for n in (1, N)}
            torch.cuda.synchronize()
            occ, rng = d_occ.cpu().numpy().reshape(N, SCENE.gh, SCENE.gw), d_rng.cpu().numpy().reshape(N, SCENE.beams)
            for n in (N, 1):
                stage.append({"n": n, "forward_us_per_pair": round(fwd[n], 3), "obstacles_us_per_map": round(ob[n], 3),
                              "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            edges = api.beam_edges(SCENE)
            d_grid = torch.empty(N * cells, dtype=torch.int8, device="cuda")
            d_log = torch.empty(N * cells, dtype=torch.int16, device="cuda")
            d_stats = torch.empty(N * 4, dtype=torch.int32, device="cuda")
            for name, n, ids in CASES:
                streams = n if ids else 1
                for what, sel in OUTPUTS.items():
                    ptrs = [t.data_ptr() if s else 0 for t, s in zip((d_grid, d_log, d_stats), sel)]
                    with eng.costmap(SCENE, MAP, streams=streams) as cm:
                        def call():
                            return cm.push_device(n, poses[:n], d_occ.data_ptr(), d_rng.data_ptr(), ids, *ptrs, stream=st.cuda_stream)
                        m = min(n, 3)      # the twin's bytes before the clock starts
                        q = cm.push_device(m, poses[:m], d_occ.data_ptr(), d_rng.data_ptr(), ids[:m] if ids else None, *ptrs)
                        twin = costmap.Reference(MAP, SCENE, streams, edges=edges)
                        want = twin.push(q, occ[:m], rng[:m], ids[:m] if ids else None)
                        for t, s, w_ in zip((d_grid, d_log, d_stats), sel, want):
                            if s and t[:w_.size].cpu().numpy().tobytes() != w_.tobytes():
                                raise SystemExit(f"{name} ({what}): differs from the numpy twin")
                        cm.reset()
                        ms = timed(call, st, args.warmup, args.iters)
                    per_frame = (cells if sel[0] else 0) + (2 * cells if sel[1] else 0) + (16 if sel[2] else 0) + ocells + 4 * SCENE.beams
                    floor_bytes = (4 * cells * streams + per_frame * n) / n
                    us, floor_us = ms * 1e3 / n, floor_bytes / HBM_BYTES_PER_S * 1e6
                    rows.append({"case": name, "outputs": what, "n": n, "streams": streams, "us": round(ms * 1e3, 3), "us_per_map": round(us, 3),
                                 "obstacles_us_per_map": round(ob[n], 3), "forward_us_per_pair": round(fwd[n], 3),
                                 "share_of_forward": round(us / fwd[n], 5), "floor_bytes_per_map": int(floor_bytes),
                                 "floor_us_per_map": round(floor_us, 4), "fraction_of_floor": round(floor_us / us, 5),
                                 "stats_of_map_0": [int(v) for v in want[2][0]]})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = {"costmap_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "window": [MAP.mw, MAP.mh], "grid": [SCENE.gw, SCENE.gh], "beams": SCENE.beams,
           "stages": stage, "costmap": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
