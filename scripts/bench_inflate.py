#!/usr/bin/env python3
"""Times the inflation of occupancy grids (device buffers, a caller stream, device events, 50 calls after 5 warm-up) on the
costmap bench's window: 400 x 400 cells of 0.05 m, at R = 8 (a 0.4 m inflation radius) and R = 32 (1.6 m), at batch 64 and at
batch 1, with all four outputs and with the grid alone.  The inputs are the costmap stage's own grids along the walk of
scripts/bench_costmap.py (obstacles.ground_and_wall scenes through sn_obstacles_from_raw and sn_costmap_push as one clip).  In
the same run, on the same box: sn_costmap_push (grid alone, one clip of 64 frames and n = 1) and sn_infer_batch per pair.  The
first three maps of every configuration are compared with the numpy twin's bytes before anything is timed.  Prints one JSON line.

    python scripts/bench_inflate.py [--iters K] [--warmup W] [--out FILE]

Under SN_INFLATE_WAVES=4 or =16 (read by sn_create) every call takes that form of the kernel instead of the one its size picks;
the line records the setting as "inflate_waves".

The byte floor per map at the achievable HBM rate (6.3 TB/s, a float4 copy on this part): per cell 1 byte of occ read plus the
bytes of the requested outputs (cost 1, grid 1, dist2 2; 20 of statistics a map).  `fraction_of_floor` = floor time / measured.
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

from hobot_stereonet_amd import api, inflate, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd.costmap import CostmapParams  # noqa: E402
from hobot_stereonet_amd.inflate import InflateParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
HBM_BYTES_PER_S = 6.3e12
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
SCENE = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15,
                       z_lo_m=0.1, z_hi_m=1.5, beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
MAP = CostmapParams(mw=400, mh=400, l_hit=85, l_miss=40, l_min=-200, l_max=350, clear_margin_m=0.1, clear_min_m=0.2, clear_max_m=0.0)
RADII = {8: InflateParams(cell_m=0.05, inscribed_radius_m=0.2, inflation_radius_m=0.4, cost_scaling=10.0, lethal_min=50, flags=0),
         32: InflateParams(cell_m=0.05, inscribed_radius_m=0.2, inflation_radius_m=1.6, cost_scaling=3.0, lethal_min=50, flags=0)}
OUTPUTS = {"all": (True, True, True, True), "grid": (False, True, False, False)}


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
    cells = MAP.mw * MAP.mh
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
            d_occ = torch.empty(N * SCENE.gw * SCENE.gh, dtype=torch.int8, device="cuda")
            d_rng = torch.empty(N * SCENE.beams, dtype=torch.float32, device="cuda")
            eng.obstacles_device(N, d_raw.data_ptr(), CAM, SCENE, occ_ptr=d_occ.data_ptr(), ranges_ptr=d_rng.data_ptr())
            d_map = torch.empty(N * cells, dtype=torch.int8, device="cuda")
            cmap = {}
            for n in (N, 1):      # the stage this one follows: the grid alone, one clip
                with eng.costmap(SCENE, MAP) as cm:
                    cmap[n] = timed(lambda: cm.push_device(n, poses[:n], d_occ.data_ptr(), d_rng.data_ptr(), None, d_map.data_ptr(), 0, 0,
                                                           stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3 / n
            with eng.costmap(SCENE, MAP) as cm:      # the maps that are inflated: the clip's 64 grids
                cm.push_device(N, poses, d_occ.data_ptr(), d_rng.data_ptr(), None, d_map.data_ptr(), 0, 0)
            torch.cuda.synchronize()
            grids = d_map.cpu().numpy().reshape(N, MAP.mh, MAP.mw)
            for n in (N, 1):
                stage.append({"n": n, "forward_us_per_pair": round(fwd[n], 3), "costmap_us_per_map": round(cmap[n], 3),
                              "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            d_cost = torch.empty(N * cells, dtype=torch.uint8, device="cuda")
            d_grid = torch.empty(N * cells, dtype=torch.int8, device="cuda")
            d_dist = torch.empty(N * cells, dtype=torch.int16, device="cuda")
            d_stats = torch.empty(N * 5, dtype=torch.int32, device="cuda")
            bufs = (d_cost, d_grid, d_dist, d_stats)
            for R, p in RADII.items():
                assert inflate.radius_cells(p) == R
                want = inflate.reference(grids[:3], p, api.inflate_table(p))
                for n in (N, 1):
                    for what, sel in OUTPUTS.items():
                        ptrs = [t.data_ptr() if s else 0 for t, s in zip(bufs, sel)]
                        m = min(n, 3)      # the twin's bytes before the clock starts
                        eng.inflate_device(m, d_map.data_ptr(), MAP.mw, MAP.mh, p, *ptrs)
                        for t, s, w_ in zip(bufs, sel, want[:4]):
                            if s and t[:w_[:m].size].cpu().numpy().tobytes() != np.ascontiguousarray(w_[:m]).tobytes():
                                raise SystemExit(f"R = {R}, n = {n} ({what}): differs from the numpy twin")
                        ms = timed(lambda: eng.inflate_device(n, d_map.data_ptr(), MAP.mw, MAP.mh, p, *ptrs, stream=st.cuda_stream), st,
                                   args.warmup, args.iters)
                        floor_bytes = cells * (1 + sel[0] + sel[1] + 2 * sel[2]) + 20 * sel[3]
                        us, floor_us = ms * 1e3 / n, floor_bytes / HBM_BYTES_PER_S * 1e6
                        rows.append({"R": R, "outputs": what, "n": n, "us": round(ms * 1e3, 3), "us_per_map": round(us, 3),
                                     "costmap_us_per_map": round(cmap[n], 3), "forward_us_per_pair": round(fwd[n], 3),
                                     "share_of_forward": round(us / fwd[n], 5), "ratio_to_costmap": round(us / cmap[n], 4),
                                     "floor_bytes_per_map": int(floor_bytes), "floor_us_per_map": round(floor_us, 4),
                                     "fraction_of_floor": round(floor_us / us, 5), "stats_of_map_0": [int(v) for v in want[3][0]],
                                     "obstacle_cells_of_map_0": int((grids[0] >= p.lethal_min).sum())})
                        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = {"inflate_bench": True, "inflate_waves": os.environ.get("SN_INFLATE_WAVES", "by size"), "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "window": [MAP.mw, MAP.mh], "cell_m": 0.05, "stages": stage, "inflate": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
