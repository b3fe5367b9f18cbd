#!/usr/bin/env python3
"""Times sn_smooth_raw (device buffers, a caller stream, device events, after warm-up) at 1280x720 for n = 1, 16 and 64, radius
1, 2 and 3, each as a plain median (sigma_luma 0) and guided (sigma_luma 12, the int8 model input as the guide), min_valid 3,
with sn_infer_batch per map at the same n on the same handle beside it (the forward is the yardstick: a setting of radius <= 2
that costs more per map than the forward at batch 64 counts as unfinished; radius 3 is reported only).  The maps are the
masked output of sn_infer_lrc on synth pairs.  Every call writes out_raw (not in place), the mask, the float map and the counts.
Prints one JSON line.

    python scripts/bench_smooth.py [--iters K] [--warmup W] [--out FILE]

The kernel is compute: (2r+1)^4 compare-select-add steps per pixel (81, 625, 2401) against 10 first-touch bytes (raw 4, luma 1,
out 4, mask 1) plus 4 per changed pixel for the float map; both rates are reported.
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

from hobot_stereonet_amd import api, synth, weights  # noqa: E402

W, H, D = 1280, 720, 192
TAU = (1.0, 0.0)
MIN_VALID = 3
SETTINGS = [(r, s) for r in (1, 2, 3) for s in (0, 12)]


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    nmax = 64
    seeds = np.stack([synth.model_input_i8(W, H, D, s) for s in range(4)])
    x = np.ascontiguousarray(np.tile(seeds, (nmax // 4, 1, 1, 1)))
    rows, forward = [], []
    with tempfile.TemporaryDirectory() as td:
        model = os.path.join(td, "m.snw")
        weights.save_snw(model, weights.synthetic(0), W, H, D)
        with api.StereoNetHIP(model, max_batch=nmax) as eng:
            dx = torch.from_numpy(x).cuda()
            lrc = torch.empty((nmax, H, W), dtype=torch.int32, device="cuda")
            disp = torch.empty((nmax, H, W), dtype=torch.float32, device="cuda")
            out = torch.empty_like(lrc)
            mask = torch.empty((nmax, H, W), dtype=torch.uint8, device="cuda")
            counts = torch.empty((nmax, 3), dtype=torch.int32, device="cuda")
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            fwd_ms = {}
            for n in (1, 16, 64):
                fwd_ms[n] = timed(lambda: eng.infer_device(n, dx.data_ptr(), out.data_ptr(), disp.data_ptr(), st.cuda_stream),
                                  st, args.warmup, args.iters)
                forward.append({"n": n, "infer_batch_ms": round(fwd_ms[n], 4), "ms_per_map": round(fwd_ms[n] / n, 4),
                                "precision": api.PREC_NAMES.get(eng.precision_selected, "?")})
            eng.infer_lrc_device(nmax, dx.data_ptr(), TAU[0], TAU[1], lrc.data_ptr(), disp.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            for radius, sigma in SETTINGS:
                for n in (1, 16, 64):
                    def call(stream=st.cuda_stream):
                        eng.smooth_raw_device(n, lrc.data_ptr(), dx.data_ptr(), api.SN_GUIDE_TENSOR, 0, radius, sigma, MIN_VALID,
                                              out_raw_ptr=out.data_ptr(), mask_ptr=mask.data_ptr(), disp_ptr=disp.data_ptr(),
                                              counts_ptr=counts.data_ptr(), stream=stream)
                    ms = timed(call, st, args.warmup, args.iters)
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        call(0)                                  # the smoother's own stream: returns after completion
                    wall = (time.perf_counter() - t0) * 1e3 / args.iters
                    c = counts[:n].cpu().numpy().view(np.uint32).astype(np.int64).sum(0)
                    px = n * H * W
                    changed = int(c[1] + c[2])
                    nbytes = (10 if sigma else 9) * px + 4 * changed
                    steps = (2 * radius + 1) ** 4 * px
                    rows.append({"radius": radius, "sigma_luma": sigma, "min_valid": MIN_VALID, "n": n, "ms": round(ms, 4),
                                 "ms_per_map": round(ms / n, 4), "own_stream_wall_ms_per_map": round(wall / n, 4),
                                 "forward_ms_per_map": round(fwd_ms[n] / n, 4), "share_of_forward": round(ms / fwd_ms[n], 4),
                                 "share_of_forward_at_64": round((ms / n) / (fwd_ms[64] / 64), 4),
                                 "valid_fraction": round(float(c[0]) / px, 4), "smoothed": int(c[1]), "filled": int(c[2]),
                                 "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                 "Gsteps_per_s": round(steps / (ms * 1e-3) / 1e9, 1)})
    line = json.dumps({"smooth_bench": True, "width": W, "height": H, "dmax": D, "gpu": torch.cuda.get_device_name(0),
                       "iters": args.iters, "warmup": args.warmup, "tau": TAU, "forward": forward, "smooth": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
