#!/usr/bin/env python3
"""Times the ground-plane stage (device buffers, a caller stream, device events, 50 calls after 5 warm-up) at 1280x720, batches 64
and 1: sn_ground_from_raw at step 1 and 2, K = 64 / 256 / 1024 hypotheses, 0 and 2 refits, with and without the labels, on the
lower half of the image; and, in the same run and on the same maps, sn_obstacles_from_raw (the grid and the scan of
bench_obstacles.py's scene parameters), the chain sn_ground_from_raw -> sn_obstacles_from_raw_mounts on one stream, and
sn_infer_batch per pair at batch 64.  The maps are ground.scene: a camera 0.4 .. 1.0 m above a floor, pitched and rolled from
map to map, a wall, boxes, 10 % outliers and 5 % holes.  The record and the labels of the first map of every (step, K, refits)
are compared with the numpy twin's bytes before anything is timed.  `parts` times the default configuration (step 2, K = 256,
two refits, no labels) with one piece taken away at a time: K = 1 (everything but the scoring), no refit, and a region of a
quarter of the rows.  Prints one JSON line.

    python scripts/bench_ground.py [--iters K] [--warmup W] [--out FILE]
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

from hobot_stereonet_amd import api, ground, obstacles, synth, weights  # noqa: E402
from hobot_stereonet_amd.ground import GroundParams  # noqa: E402
from hobot_stereonet_amd.obstacles import ObstacleParams  # noqa: E402
from hobot_stereonet_amd.pointcloud import Camera  # noqa: E402

W, H, D = 1280, 720, 192
N = 64
CAM = Camera(fx=1066.0, fy=1066.0, cx=639.5, cy=273.5, baseline_mm=120.0)
BASE = GroundParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), hypotheses=256, seed=1, refits=2, tol_px=0.1, min_inliers=5000, min_area=4096,
                    max_tilt_rad=0.5, height_min_m=0.2, height_max_m=2.0)
OB = ObstacleParams(x_min_m=0.0, y_min_m=-5.0, cell_m=0.05, gw=200, gh=200, z_floor_m=-0.15, z_lo_m=0.1, z_hi_m=1.5, beams=360, angle_min_rad=-0.54,
                    angle_increment_rad=0.003, range_min_m=0.2, range_max_m=20.0)


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
    rng = np.random.default_rng(0)
    scene = np.stack([ground.scene(W, H, CAM, rng.uniform(0.4, 1.0), rng.uniform(0.0, 0.3), rng.uniform(-0.1, 0.1), wall_z_m=rng.uniform(6.0, 15.0),
                                   boxes=3, hole_frac=0.05, outlier_frac=0.10, seed=k)[0] for k in range(N)])
    frames = np.stack([synth.sbs_nv12_frame(W, H, D, 21 + k).reshape(-1) for k in range(4)])
    rows, parts = [], []
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
            del dx, d_sbs, d_net
            d_raw = torch.from_numpy(scene).cuda()
            d_rec = torch.zeros(N * ground.RECORD.itemsize, dtype=torch.uint8, device="cuda")
            d_lab = torch.empty(N * H * W, dtype=torch.uint8, device="cuda")
            cells = OB.gw * OB.gh
            ob_bufs = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in (N * cells, N * cells * 8, N * cells * 4, N * OB.beams * 4, N * 16)]
            ob_ptrs = [b.data_ptr() for b in ob_bufs]
            level = dataclasses.replace(OB, base_from_cam=BASE.base_from_cam)
            ob_us = {n: timed(lambda: eng.obstacles_device(n, d_raw.data_ptr(), CAM, level, *ob_ptrs, stream=st.cuda_stream), st, args.warmup,
                              args.iters) * 1e3 / n for n in (N, 1)}
            found = {}
            for step in (1, 2):
                cam = dataclasses.replace(CAM, step=step)
                for K in (64, 256, 1024):
                    for refits in (0, 2):
                        p = dataclasses.replace(BASE, hypotheses=K, refits=refits, min_inliers=BASE.min_inliers // (step * step))
                        eng.ground_device(N, d_raw.data_ptr(), cam, p, d_rec.data_ptr(), d_lab.data_ptr())
                        rec = d_rec.cpu().numpy().view(ground.RECORD)
                        want, wlab = ground.reference(scene[0], cam, p, gate_q16=api.ground_gate(cam, p, W, H))
                        if rec[0].tobytes() != want.tobytes() or not np.array_equal(d_lab[:H * W].cpu().numpy().reshape(H, W), wlab):
                            raise SystemExit(f"step {step}, K {K}, refits {refits}: the first map's outputs differ from the numpy twin")
                        found[(step, K, refits)] = int(np.count_nonzero(rec["flags"] & ground.FOUND))
                        for labels in (False, True):
                            for n in (N, 1):
                                ms = timed(lambda: eng.ground_device(n, d_raw.data_ptr(), cam, p, d_rec.data_ptr(), d_lab.data_ptr() if labels else 0,
                                                                     stream=st.cuda_stream), st, args.warmup, args.iters)
                                us = ms * 1e3 / n
                                rows.append({"step": step, "hypotheses": K, "refits": refits, "labels": labels, "n": n, "us_per_map": round(us, 3),
                                             "obstacles_us_per_map": round(ob_us[n], 3), "over_obstacles": round(us / ob_us[n], 3),
                                             "forward_us_per_pair": fwd["us_per_pair"], "share_of_forward": round(us / fwd["us_per_pair"], 5),
                                             "launches": 6 + 2 * refits + labels, "found_of_64": found[(step, K, refits)]})
                                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            # where the default configuration's time goes, and the chain on one stream
            cam = dataclasses.replace(CAM, step=2)
            dflt = dataclasses.replace(BASE, min_inliers=BASE.min_inliers // 4)
            mounts = d_rec.data_ptr() + 4 * ground.MOUNT_OFFSET_FLOATS

            def chain(n):
                eng.ground_device(n, d_raw.data_ptr(), cam, dflt, d_rec.data_ptr(), 0, stream=st.cuda_stream)
                eng.obstacles_device(n, d_raw.data_ptr(), CAM, OB, *ob_ptrs, stream=st.cuda_stream, mounts_ptr=mounts, mount_stride=ground.RECORD_FLOATS)

            for what, p in (("default", dflt), ("one hypothesis: everything but the scoring", dataclasses.replace(dflt, hypotheses=1)),
                            ("no refit", dataclasses.replace(dflt, refits=0)),
                            ("a quarter of the rows", dataclasses.replace(dflt, roi_x=0, roi_y=H // 2, roi_w=W, roi_h=H // 8))):
                for n in (N, 1):
                    ms = timed(lambda: eng.ground_device(n, d_raw.data_ptr(), cam, p, d_rec.data_ptr(), 0, stream=st.cuda_stream), st, args.warmup, args.iters)
                    parts.append({"what": what, "n": n, "us_per_map": round(ms * 1e3 / n, 3)})
                    print(json.dumps(parts[-1]), file=sys.stderr, flush=True)
            for n in (N, 1):
                ms = timed(lambda: chain(n), st, args.warmup, args.iters)
                parts.append({"what": "ground then obstacles with the fitted mounts, one stream", "n": n, "us_per_map": round(ms * 1e3 / n, 3),
                              "obstacles_alone_us_per_map": round(ob_us[n], 3)})
                print(json.dumps(parts[-1]), file=sys.stderr, flush=True)
    out = {"ground_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "forward": fwd, "ground": rows, "parts": parts}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
