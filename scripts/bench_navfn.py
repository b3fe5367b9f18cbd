#!/usr/bin/env python3
"""Times the navigation function and path (sn_navfn) on the inflation bench's window: 400 x 400 cells of 0.05 m, the costmap
stage's own grids along the walk of scripts/bench_costmap.py inflated at R = 8 (scripts/bench_inflate.py's set-up), the start
at the centre of the window (the robot's cell) and the goal near its far edge, unknown cells passable.  Device buffers, 50 calls
after 5 warm-up, at batch 64 and at batch 1:

  converge   max_rounds = 0: the call reads its work word back every few rounds and returns after completion, so it is timed by
             the host's clock around the call; also how many rounds did work.
  fixed      max_rounds = what the converging call reported plus one, on a caller stream, device events: nothing but enqueues;
             and the same with the potential alone (no starts, no path, no stats), which leaves init and the rounds.

In the same run, on the same box: sn_infer_batch per pair, sn_inflate_grid per map (the cost alone), and the thing this stage
replaces: a plain binary-heap Dijkstra in C++ on one host thread (navfn_harness --bench) over map 0's costs.  The first three
maps are compared with the heapq twin's bytes before anything is timed.  Prints one JSON line.

    python scripts/bench_navfn.py [--iters K] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, navfn, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd.costmap import CostmapParams  # noqa: E402
from hobot_stereonet_amd.inflate import InflateParams  # noqa: E402
from hobot_stereonet_amd.navfn import NavParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
SCENE = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15,
                       z_lo_m=0.1, z_hi_m=1.5, beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
MAP = CostmapParams(mw=400, mh=400, l_hit=85, l_miss=40, l_min=-200, l_max=350, clear_margin_m=0.1, clear_min_m=0.2, clear_max_m=0.0)
INFLATION = InflateParams(cell_m=0.05, inscribed_radius_m=0.2, inflation_radius_m=0.4, cost_scaling=10.0, lethal_min=50, flags=0)      # R = 8
PLAN = NavParams(neutral=50, lethal_cost=253, unknown_cost=20, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=2048)
HARNESS = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat", "build", "navfn_harness")


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
    gw, gh = MAP.mw, MAP.mh
    cells = gw * gh
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
            with eng.costmap(SCENE, MAP) as cm:      # the clip's 64 grids
                cm.push_device(N, poses, d_occ.data_ptr(), d_rng.data_ptr(), None, d_map.data_ptr(), 0, 0)
            d_cost = torch.empty(N * cells, dtype=torch.uint8, device="cuda")
            eng.inflate_device(N, d_map.data_ptr(), gw, gh, INFLATION, cost_ptr=d_cost.data_ptr())
            torch.cuda.synchronize()
            infl = {n: timed(lambda: eng.inflate_device(n, d_map.data_ptr(), gw, gh, INFLATION, cost_ptr=d_cost.data_ptr(), stream=st.cuda_stream),
                             st, args.warmup, args.iters) * 1e3 / n for n in (N, 1)}
            cost = d_cost.cpu().numpy().reshape(N, gh, gw)
            # the robot stands at the centre of its window; the goal is the passable cell nearest to 15 cells short of the far edge
            passable = navfn.weights(cost, PLAN) > 0
            starts = np.tile(np.array([[gw // 2, gh // 2]], np.int32), (N, 1))
            goals = np.empty((N, 2), np.int32)
            for k in range(N):
                ys, xs = np.nonzero(passable[k])
                i = int(np.argmin((xs - (gw - 15)) ** 2 + (ys - gh // 2) ** 2))
                goals[k] = (xs[i], ys[i])
            d_goals, d_starts = torch.from_numpy(goals).cuda(), torch.from_numpy(starts).cuda()
            d_pot = torch.empty(N * cells, dtype=torch.int32, device="cuda")
            d_path = torch.full((N * PLAN.max_path * 2,), -1, dtype=torch.int32, device="cuda")
            d_stats = torch.empty(N * 5, dtype=torch.int32, device="cuda")
            ptrs = (d_pot.data_ptr(), d_path.data_ptr(), d_stats.data_ptr())

            def call(n, p, stream=0):
                return eng.navfn_device(n, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), d_starts.data_ptr(), p, *ptrs, stream=stream)

            want = navfn.reference(cost[:3], goals[:3], starts[:3], PLAN)      # the twin's bytes before the clock starts
            call(3, PLAN)
            torch.cuda.synchronize()
            got_path = d_path[:3 * PLAN.max_path * 2].cpu().numpy().reshape(3, PLAN.max_path, 2)
            if (d_pot[:3 * cells].cpu().numpy().view(np.uint32).tobytes() != want[0].tobytes() or got_path.tobytes() != want[1].tobytes()
                    or d_stats[:15].cpu().numpy().view(np.uint32).tobytes() != want[2].tobytes()):
                raise SystemExit("sn_navfn differs from the heapq twin")
            cost[0].tofile(os.path.join(td, "cost0.bin"))
            host = json.loads(subprocess.run([HARNESS, "--bench", os.path.join(td, "cost0.bin"), str(gw), str(gh), str(goals[0, 0]), str(goals[0, 1]),
                                              str(PLAN.neutral), str(PLAN.lethal_cost), str(PLAN.unknown_cost if PLAN.flags & navfn.UNKNOWN_OK else -1), "20"], check=True, capture_output=True, text=True).stdout)
            for n in (N, 1):
                for _ in range(args.warmup):
                    rounds = call(n, PLAN)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    rounds = call(n, PLAN)
                conv_us = (time.perf_counter() - t0) / args.iters * 1e6
                fixed = NavParams(**{**PLAN.__dict__, "max_rounds": rounds + 1})
                call(n, fixed)
                torch.cuda.synchronize()
                flags = d_stats[:5 * n].cpu().numpy().reshape(n, 5)[:, 0]
                fixed_us = timed(lambda: call(n, fixed, st.cuda_stream), st, args.warmup, args.iters) * 1e3
                st_host = d_stats[:5 * n].cpu().numpy().view(np.uint32).reshape(n, 5)
                field_us = timed(lambda: eng.navfn_device(n, d_cost.data_ptr(), gw, gh, d_goals.data_ptr(), 0, fixed, d_pot.data_ptr(), 0, 0,
                                                          stream=st.cuda_stream), st, args.warmup, args.iters) * 1e3
                rows.append({"n": n, "rounds": int(rounds), "converge_us": round(conv_us, 2), "converge_us_per_map": round(conv_us / n, 3),
                             "fixed_rounds": int(rounds + 1), "fixed_us": round(fixed_us, 2), "fixed_us_per_map": round(fixed_us / n, 3),
                             "fixed_field_only_us": round(field_us, 2), "fixed_field_only_us_per_round": round(field_us / (rounds + 1), 3),
                             "path_and_stats_us": round(fixed_us - field_us, 2), "fixed_unconverged_maps": int(np.count_nonzero(flags & navfn.UNCONVERGED)),
                             "path_cells_of_map_0": int(st_host[0, 2]), "reached_of_map_0": int(st_host[0, 1]),
                             "inflate_us_per_map": round(infl[n], 3), "forward_us_per_pair": round(fwd[n], 3),
                             "host_dijkstra_us_per_map": host["dijkstra_us"],
                             "ratio_to_host_dijkstra": round(fixed_us / n / host["dijkstra_us"], 4)})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                stage.append({"n": n, "forward_us_per_pair": round(fwd[n], 3), "inflate_us_per_map": round(infl[n], 3),
                              "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
    out = {"navfn_bench": True, "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "window": [gw, gh], "cell_m": 0.05,
           "tile": [navfn.TILE_W, navfn.TILE_H], "params": {k: v for k, v in PLAN.__dict__.items() if k not in ("goal", "start")},
           "host_dijkstra": host, "stages": stage, "navfn": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
