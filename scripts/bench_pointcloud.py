#!/usr/bin/env python3
"""Times sn_pointcloud_from_raw (device mode, device events, after warm-up) on seeded 1280x720 maps with ~80 % valid
samples: n = 1 and n = 64, both layouts, with and without colour (side-by-side NV12 frames, pitch 2W); plus host mode at
n = 1 (the node's call: H2D of the map and frame, D2H of the cloud, wall clock).  Prints one JSON line.

    python scripts/bench_pointcloud.py [--iters K] [--warmup W] [--out FILE]

Algorithmic bytes per call, from shapes and the returned counts (S samples, V valid points):
    organised  S * (4 raw + 16 point [+ 1.5 NV12])
    compact    S * 8 (raw in both passes) + V * (16 point [+ 1.5 NV12])
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  first HIP-linked import (api.load_library)

from hobot_stereonet_amd import api, pointcloud, weights  # noqa: E402
from hobot_stereonet_amd.pointcloud import COMPACT, ORGANISED, Camera  # noqa: E402

W, H, D = 1280, 720, 192


def seeded(n):
    rng = np.random.default_rng(2026)
    raw = rng.integers(40000, 600000, (n, H, W)).astype(np.int32)
    raw[rng.random((n, H, W)) < 0.2] = 0
    nv12 = rng.integers(0, 256, n * pointcloud.nv12_frame_bytes(2 * W, H), dtype=np.uint8)
    return raw, nv12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    cam = Camera()
    results = []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=64) as eng:
            for n in (1, 64):
                raw, nv12 = seeded(n)
                draw = torch.from_numpy(raw).cuda()
                dnv = torch.from_numpy(nv12).cuda()
                pts = torch.empty((n, H * W, 4), dtype=torch.float32, device="cuda")
                cnt = torch.empty(n, dtype=torch.int32, device="cuda")
                st = torch.cuda.Stream()
                for layout in (ORGANISED, COMPACT):
                    for colour in (False, True):
                        def call():
                            eng.pointcloud_device(n, draw.data_ptr(), cam, pts.data_ptr(), cnt.data_ptr(),
                                                  dnv.data_ptr() if colour else 0, 2 * W if colour else 0, layout,
                                                  st.cuda_stream)
                        for _ in range(args.warmup):
                            call()
                        st.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        for _ in range(args.iters):
                            call()
                        e1.record(st)
                        e1.synchronize()
                        ms = e0.elapsed_time(e1) / args.iters
                        s = n * H * W
                        v = int(cnt.cpu().numpy().view(np.uint32).astype(np.int64).sum())
                        c = 1.5 if colour else 0.0
                        nbytes = s * (20 + c) if layout == ORGANISED else s * 8 + v * (16 + c)
                        results.append({"mode": "device", "n": n, "layout": "organised" if layout == ORGANISED else "compact",
                                        "colour": colour, "ms": round(ms, 4), "valid_fraction": round(v / s, 4),
                                        "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)})
                del draw, dnv, pts, cnt
                torch.cuda.empty_cache()
            raw, nv12 = seeded(1)
            for layout in (ORGANISED, COMPACT):
                for _ in range(args.warmup):
                    eng.pointcloud(raw[0], cam, layout, nv12, 2 * W)
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    eng.pointcloud(raw[0], cam, layout, nv12, 2 * W)
                ms = (time.perf_counter() - t0) / args.iters * 1e3
                results.append({"mode": "host", "n": 1, "layout": "organised" if layout == ORGANISED else "compact",
                                "colour": True, "ms": round(ms, 4)})
    line = json.dumps({"pointcloud_bench": True, "width": W, "height": H, "gpu": torch.cuda.get_device_name(0),
                       "iters": args.iters, "warmup": args.warmup, "results": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
