#!/usr/bin/env python3
"""Times the obstacle grid and laser scan (device buffers, a caller stream, device events, 50 calls after 5 warm-up) at 1280x720,
batches 64 and 1: sn_obstacles_from_raw with all five outputs in its run-length form and in its plain form (SN_OBSTACLE_RLE=0,
one set of atomics per point; an engine of its own, the switch is read by sn_create) and, in the same run and on the same maps,
the yardstick sn_pointcloud_from_raw (organised, no colour, step 1: it reads the same words and writes 16 bytes a point where
this stage writes almost nothing, so any time above it is the price of the atomics) and sn_infer_batch per pair at batch 64.
Three inputs: `scene`, obstacles.ground_and_wall scaled up (a level camera 0.5 m above the ground, a wall at 3.1 m and farther
from map to map); `network`, the engine's own maps of synth.sbs_nv12_frame pairs under parameters fitted to their depths; and
`one cell`, the worst case for contention, a constant map whose every pixel hits one cell and one beam.  Every output of both
forms is compared with the numpy twin's bytes on the first map before it is timed; `parts` times the run-length form on the
scene with the grid alone, the scan alone, and bands that hold no point.  Prints one JSON line.

    python scripts/bench_obstacles.py [--iters K] [--warmup W] [--out FILE]

The byte floor per map at the achievable HBM rate (6.3 TB/s, a float4 copy on this part): the map read once (4 W H) plus the
outputs written once (13 bytes a cell, 4 a beam, 16 of statistics).  `fraction_of_floor` = floor time / measured.
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
HBM_BYTES_PER_S = 6.3e12
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
LEVEL = obstacles.mount(t=(0.0, 0.0, 0.5))
SCENE = ObstacleParams(base_from_cam=LEVEL, x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15, z_lo_m=0.1, z_hi_m=1.5,
                       beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)
ONE_CELL = ObstacleParams(x_min_m=-64.0, y_min_m=-64.0, cell_m=128.0, gw=1, gh=1, z_floor_m=-50.0, z_lo_m=-40.0, z_hi_m=50.0, beams=1,
                          angle_min_rad=-1.2, angle_increment_rad=2.4, range_min_m=0.0, range_max_m=1000.0)


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


def fitted(raw):
    """parameters whose grid and bands are percentiles of the map's own base-frame coordinates: the network's maps of synthetic
    weights have no scene in them, this gives the stage a realistic spread of cells and beams on them"""
    xb, yb, zb = obstacles.base_points(raw, CAM, ObstacleParams(base_from_cam=LEVEL))
    ok = np.isfinite(xb)
    q = lambda a, pc: float(np.float32(np.percentile(a[ok].astype(np.float64), pc)))      # noqa: E731
    x0, x1, y0, y1 = q(xb, 5), q(xb, 95), q(yb, 5), q(yb, 95)
    cell = float(np.float32(max((x1 - x0) / 200, (y1 - y0) / 200, 1e-3)))
    return ObstacleParams(base_from_cam=LEVEL, x_min_m=x0, y_min_m=y0, cell_m=cell, gw=200, gh=200, z_floor_m=q(zb, 5), z_lo_m=q(zb, 40),
                          z_hi_m=q(zb, 95), beams=360, angle_min_rad=-0.54, angle_increment_rad=0.003, range_min_m=0.0,
                          range_max_m=float(np.float32(2 * x1 + 1)))


def outputs(p):
    cells = p.gw * p.gh
    sizes = (N * cells, N * cells * 8, N * cells * 4, N * p.beams * 4, N * 16)
    return [torch.empty(max(s, 16), dtype=torch.uint8, device="cuda") for s in sizes], sizes


def check(eng, name, form, d_raw, raw0, p, bufs, sizes):
    eng.obstacles_device(1, d_raw.data_ptr(), CAM, p, *[b.data_ptr() for b in bufs])
    want = obstacles.reference(raw0, CAM, p, edges=api.beam_edges(p))
    for what, b, s, w_ in zip(("occ", "hits", "height_mm", "ranges", "stats"), bufs, sizes, want):
        if b[:s // N].cpu().numpy().tobytes() != np.ascontiguousarray(w_).tobytes():
            raise SystemExit(f"{name} ({form}): {what} differs from the numpy twin")
    return [int(v) for v in want[4]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    scene = np.stack([obstacles.ground_and_wall(W, H, CAM, 0.5, 3.1 + 0.11 * k) for k in range(N)])
    const = np.full((N, H, W), 9000, np.int32)
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)])
    rows_out, parts, stats = [], [], {}
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
            fwd_ms = timed(lambda: eng.infer_device(N, dx.data_ptr(), d_net.data_ptr(), 0, st.cuda_stream), st, 3, 20)
            fwd = {"n": N, "infer_batch_ms": round(fwd_ms, 4), "us_per_pair": round(fwd_ms * 1e3 / N, 3),
                   "precision": api.PREC_NAMES.get(eng.precision_selected, "?")}
            del dx, d_sbs
            net0 = d_net[0].cpu().numpy()
            inputs = {"scene": (torch.from_numpy(scene).cuda(), scene[0], SCENE), "network": (d_net, net0, fitted(net0)),
                      "one cell": (torch.from_numpy(const).cuda(), const[0], ONE_CELL)}
            d_pts = torch.empty((N, H, W, 4), dtype=torch.float32, device="cuda")
            pc = {}
            for name, (d_raw, _, _) in inputs.items():
                for n in (N, 1):
                    ms = timed(lambda: eng.pointcloud_device(n, d_raw.data_ptr(), CAM, d_pts.data_ptr(), 0, stream=st.cuda_stream), st,
                               args.warmup, args.iters)
                    pc[(name, n)] = ms * 1e3 / n
            del d_pts

            def run(e, form):
                for name, (d_raw, raw0, p) in inputs.items():
                    bufs, sizes = outputs(p)
                    stats[name] = check(e, name, form, d_raw, raw0, p, bufs, sizes)
                    floor_bytes = 4 * W * H + sum(sizes) // N
                    for n in (N, 1):
                        ms = timed(lambda: e.obstacles_device(n, d_raw.data_ptr(), CAM, p, *[b.data_ptr() for b in bufs], stream=st.cuda_stream),
                                   st, args.warmup, args.iters)
                        us, floor_us = ms * 1e3 / n, floor_bytes / HBM_BYTES_PER_S * 1e6
                        rows_out.append({"input": name, "form": form, "n": n, "us_per_map": round(us, 3),
                                         "pointcloud_us_per_map": round(pc[(name, n)], 3), "over_pointcloud": round(us / pc[(name, n)], 3),
                                         "forward_us_per_pair": fwd["us_per_pair"], "share_of_forward": round(us / fwd["us_per_pair"], 4),
                                         "floor_bytes_per_map": int(floor_bytes), "floor_us_per_map": round(floor_us, 3),
                                         "fraction_of_floor": round(floor_us / us, 5), "cells": p.gw * p.gh, "beams": p.beams,
                                         "stats_of_map_0": stats[name]})
                        print(json.dumps(rows_out[-1]), file=sys.stderr, flush=True)

            run(eng, "run-length")
            # where the time of the run-length form goes, on the scene at batch 64: the grid alone, the scan alone, and the
            # walk alone (bands that hold no point: the read, the depth, the base frame and the class, no cell and no atomic)
            d_raw, _, p = inputs["scene"]
            bufs, _ = outputs(p)
            ptrs = [b.data_ptr() for b in bufs]
            nothing = dataclasses.replace(p, z_floor_m=-102.0, z_lo_m=-101.0, z_hi_m=-100.0)
            for what, prm, out in (("grid only", p, ptrs[:3] + [0, ptrs[4]]), ("scan only", p, [0, 0, 0, ptrs[3], 0]), ("no point in a band", nothing, ptrs)):
                ms = timed(lambda: eng.obstacles_device(N, d_raw.data_ptr(), CAM, prm, *out, stream=st.cuda_stream), st, args.warmup, args.iters)
                parts.append({"input": "scene", "form": "run-length", "n": N, "outputs": what, "us_per_map": round(ms * 1e3 / N, 3)})
                print(json.dumps(parts[-1]), file=sys.stderr, flush=True)
            os.environ["SN_OBSTACLE_RLE"] = "0"
            try:
                with api.StereoNetHIP(model, max_batch=N) as plain:
                    run(plain, "plain")
            finally:
                del os.environ["SN_OBSTACLE_RLE"]
    out = {"obstacle_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "forward": fwd, "obstacles": rows_out, "parts": parts}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
